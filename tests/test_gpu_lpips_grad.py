"""GPU: the backward kernels of the differentiable LPIPS, each through the C ABI with a guard region behind its output, the
whole path (LPIPS.loss) against autograd through the fp64 restatement within 4 x the fp32 composition's own error
(tests/test_lpips_grad.py: BASE), its exact properties (value bit-identical to net(x, y), run-to-run and batch invariance),
graph capture, and the latent projector on a synthetic 64-px generator."""
import pytest
import torch
import torch.nn.functional as F

from tests.lpips_f64 import synthetic_state_dict
from tests.test_lpips_grad import CASES, bound, images, reference, rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0
GUARD = 1024
U = 2.0 ** -24          # unit roundoff of fp32


def _lib():
    from rick_amd import _lib
    return _lib


def _guarded(numel):
    return torch.full((numel + GUARD,), SENTINEL, device=DEV)


def _take(buf, shape):
    n = 1
    for d in shape:
        n *= d
    assert torch.all(buf[n:] == SENTINEL), 'the kernel wrote behind its output'
    return buf[:n].view(shape).cpu()


@pytest.fixture(scope='module')
def sd():
    return synthetic_state_dict(0)


@pytest.fixture(scope='module')
def net32(sd):
    from rick_amd.lpips import LPIPS
    return LPIPS.load(sd, device=DEV, batch=3, size=32)


# ---- tap-distance backward ------------------------------------------------------------------------------------------------
def _inorm(f):
    s = (f * f).sum(-1)
    return torch.where(s > 0, 1.0 / (s.sqrt() + 1e-10), torch.zeros_like(s))


def _tap_bwd(a, ia, t, it, w, go, relu=0):
    L = _lib()
    n, HW, C = a.shape
    out = _guarded(a.numel())
    dev = [v.to(DEV).contiguous() for v in (a, ia, t, it, w, go)]
    L.check(L.lib.rick_lpips_tap_bwd_f32(*[v.data_ptr() for v in dev[:4]], n, t.shape[0], dev[4].data_ptr(), dev[5].data_ptr(), HW,
                                         C, relu, out.data_ptr(), L.stream_ptr()), 'rick_lpips_tap_bwd_f32')
    return _take(out, (n, HW, C))


@pytest.mark.parametrize('broadcast', [False, True])
@pytest.mark.parametrize('HW', [1, 7, 256])
@pytest.mark.parametrize('C', [64, 512])
def test_tap_backward_vs_fp64(C, HW, broadcast):
    """Bound, relative to the gradient's max-norm: every g_k = ia r_k - a_k q is a dozen correctly rounded operations on
    terms no larger than max |ia r| (a_k ia <= 1), plus the error of the wave's sum s = sum_c r_c a_c: an fma chain of C / 64
    terms and a six-level butterfly, at most (C / 64 + 6) U sum |r_c a_c| <= 14 U sqrt(C) max |r| / ia (Cauchy-Schwarz with
    |a| ia <= 1); the fp32 inverse norms the kernel is given carry sqrt(C) U at the worst.  (16 + 14 sqrt(C)) U covers both."""
    g = torch.Generator().manual_seed(C + HW)
    n = 3
    a = torch.relu(torch.randn(n, HW, C, generator=g))
    t = torch.relu(torch.randn(1 if broadcast else n, HW, C, generator=g))
    a[1, HW // 2] = 0                                                   # an all-zero position
    ia, it = _inorm(a), _inorm(t)
    w = torch.rand(C, generator=g) * 0.1
    go = torch.tensor([0.7, -1.3, 2.0])
    got = _tap_bwd(a, ia, t, it, w, go)
    ad = a.double().requires_grad_(True)
    na = ad / (ad.pow(2).sum(-1, keepdim=True).sqrt() + 1e-10)
    nt = t.double() * it.double()[..., None]
    val = (((na - nt) ** 2 * w.double()).sum(-1).mean(-1) * go.double()).sum()
    ref, = torch.autograd.grad(val, ad)
    live = ia > 0
    assert int((~live).sum()) == 1 and torch.all(got[~live] == 0)       # exactly 0 where ia = 0 (fp64 autograd has 0 / 0 there)
    err = float((got.double() - ref)[live].abs().max() / ref[live].abs().max())
    print(f'tap backward C={C} HW={HW} broadcast={broadcast}: {err:.3e} (bound {(16 + 14 * C ** 0.5) * U:.3e})')
    assert err <= (16 + 14 * C ** 0.5) * U
    # the ReLU form is the mask of the same values
    assert torch.equal(_tap_bwd(a, ia, t, it, w, go, relu=1), torch.where(a > 0, got, torch.zeros_like(got)))
    # the image is the target: exactly 0
    same = _tap_bwd(a, ia, a[:1] if broadcast else a, ia[:1] if broadcast else ia, w, go)
    assert torch.all(same[0] == 0) and (broadcast or torch.all(same == 0))


def test_tap_backward_refuses_bad_arguments():
    L = _lib()
    x = torch.zeros(4 * 64, device=DEV)
    p = x.data_ptr()
    args = lambda n, nt, HW, C: (p, p, p, p, n, nt, p, p, HW, C, 0, p, L.stream_ptr())
    assert L.lib.rick_lpips_tap_bwd_f32(*args(2, 3, 1, 64)) == 22        # neither n targets nor 1
    assert L.lib.rick_lpips_tap_bwd_f32(*args(1, 1, 1, 62)) == 22
    assert L.lib.rick_lpips_tap_bwd_f32(*args(1, 1, 0, 64)) == 22
    assert L.lib.rick_lpips_tap_bwd_f32(*args(1, 1, 1, 2048)) == 22
    assert L.lib.rick_lpips_maxpool2_bwd_f32(p, None, p, p, 1, 1, 4, 64, L.stream_ptr()) == 22
    assert L.lib.rick_lpips_maxpool2_bwd_f32(p, None, p, p, 1, 2, 2, 6, L.stream_ptr()) == 22
    assert L.lib.rick_lpips_input_bwd_f32(p, None, 1, 2, 2, L.stream_ptr()) == 22
    assert L.lib.rick_inc_conv_bwd_f32(p, p, None, None, None, L.stream_ptr()) == 22


# ---- convolution data gradient --------------------------------------------------------------------------------------------
_conv_refs = {}


def _conv_case(ci, co, hw):
    """Gradient GEMM with ci input and co output channels = the forward convolution co -> ci.  Computed once per case:
    (gout, forward weight, activation, add, fp64 conv_transpose2d, fp64 sum of the terms' magnitudes)."""
    key = (ci, co, hw)
    if key not in _conv_refs:
        g = torch.Generator().manual_seed(ci * 7 + co + hw[0])
        n = 3
        wf = torch.randn(ci, co, 3, 3, generator=g) * (2.0 / (9 * co)) ** 0.5
        gout = torch.randn(n, ci, *hw, generator=g)
        act = torch.relu(torch.randn(n, co, *hw, generator=g))
        add = torch.randn(n, co, *hw, generator=g)
        ref = F.conv_transpose2d(gout.double(), wf.double(), None, 1, 1)
        mag = F.conv_transpose2d(gout.double().abs(), wf.double().abs(), None, 1, 1)
        _conv_refs[key] = (gout, wf, act, add, ref, mag)
    return _conv_refs[key]


@pytest.mark.parametrize('use_mask,use_add', [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize('hw', [(1, 1), (4, 4), (9, 5)])
@pytest.mark.parametrize('ci,co', [(64, 3), (64, 64), (128, 64), (512, 256)])
def test_conv_data_gradient_vs_fp64(ci, co, hw, use_mask, use_add):
    """Every output is a sum of K = 9 ci exact fp32 products (and `add`) accumulated in fp32 in some fixed order: whatever the
    order, |error| <= (K + 1) U (sum |g| |W| + |add|) per element.  Masked elements are exactly 0."""
    from rick_amd import gemm_conv
    from rick_amd.vgg_trunk import pack_transposed
    gout, wf, act, add, ref, mag = _conv_case(ci, co, hw)
    n, (h, w) = gout.shape[0], hw
    cop_ = -(-co // 4) * 4                                               # the image's 3 channels travel as 4
    wt, cop, bn = pack_transposed(F.pad(wf, (0, 0, 0, 0, 0, cop_ - co)))

    def nhwc(t):
        return F.pad(t, (0, 0, 0, 0, 0, cop_ - co)).permute(0, 2, 3, 1).contiguous().to(DEV)
    gd, wd = gout.permute(0, 2, 3, 1).contiguous().to(DEV), wt.to(DEV)
    md, ad = (nhwc(act) if use_mask else None), (nhwc(add) if use_add else None)
    out = _guarded(n * h * w * cop_)
    a = gemm_conv.descriptor(n, h, w, ci, (3, 3), (1, 1), (1, 1), cop, bn, [(out.data_ptr(), cop_, 0, cop_)])
    gemm_conv.backward(gd.data_ptr(), wd.data_ptr(), None if md is None else md.data_ptr(), None if ad is None else ad.data_ptr(), a)
    got = _take(out, (n, h, w, cop_)).permute(0, 3, 1, 2)
    if cop_ != co:
        pad = got[:, co:]
        assert torch.all(pad == 0)                                       # the zero filter column
        got = got[:, :co]
    want, slack = ref, mag
    if use_add:
        want, slack = want + add.double(), slack + add.double().abs()
    if use_mask:
        assert torch.all(got[act <= 0] == 0)
        want, slack = torch.where(act > 0, want, torch.zeros_like(want)), torch.where(act > 0, slack, torch.zeros_like(slack))
    excess = float(((got.double() - want).abs() - (9 * ci + 1) * U * slack).max())
    print(f'conv gradient {ci}->{co} {hw} mask={use_mask} add={use_add}: max |d| {float((got.double() - want).abs().max()):.3e} '
          f'of {float(want.abs().max()):.3e}')
    assert excess <= 0


# ---- pool backward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_add', [True, False])
@pytest.mark.parametrize('hw', [(2, 2), (5, 7), (16, 16)])
def test_pool_backward_vs_torch(hw, use_add):
    L = _lib()
    g = torch.Generator().manual_seed(hw[0] * 31 + hw[1])
    n, C, (h, w) = 2, 64, hw
    act = torch.relu(torch.randn(n, C, h, w, generator=g))
    act[0, :8, 0:2, 0:2] = 1.5                                            # four equal positive values: the first takes it
    act[1, :, 0:2, 0:2] = 0                                               # an all-zero window
    add = torch.randn(n, C, h, w, generator=g)
    gpool = torch.randn(n, C, h // 2, w // 2, generator=g)
    ad = act.double().requires_grad_(True)
    adj, = torch.autograd.grad(F.max_pool2d(ad, 2, 2), ad, gpool.double())
    ref = torch.where(act > 0, (add if use_add else torch.zeros_like(add)) + adj.float(), torch.zeros_like(add))   # one fp32 add
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(DEV)
    out = _guarded(act.numel())
    actd, addd, gpd = nhwc(act), nhwc(add), nhwc(gpool)
    L.check(L.lib.rick_lpips_maxpool2_bwd_f32(actd.data_ptr(), addd.data_ptr() if use_add else None, gpd.data_ptr(), out.data_ptr(),
                                              n, h, w, C, L.stream_ptr()), 'rick_lpips_maxpool2_bwd_f32')
    got = _take(out, (n, h, w, C)).permute(0, 3, 1, 2)
    assert torch.equal(got, ref)
    base = add if use_add else torch.zeros_like(add)
    assert torch.equal(got[0, :8, 0, 0], (base + gpool[..., :1, :1])[0, :8, 0, 0])
    assert torch.equal(got[0, :8, 0, 1], base[0, :8, 0, 1]) and torch.equal(got[0, :8, 1, 1], base[0, :8, 1, 1])
    assert torch.all(got[1, :, 0:2, 0:2] == 0)
    if h % 2:                                                             # the row the floor leaves out: only `add`
        assert torch.equal(got[:, :, h - 1], torch.where(act > 0, base, torch.zeros_like(base))[:, :, h - 1])


# ---- input backward -------------------------------------------------------------------------------------------------------
def test_input_backward_is_bit_exact():
    from rick_amd.lpips import SCALE
    L = _lib()
    n, h, w = 2, 17, 23
    g = torch.randn(n, h, w, 4, generator=torch.Generator().manual_seed(0))
    out = _guarded(n * 3 * h * w)
    gd = g.to(DEV)
    L.check(L.lib.rick_lpips_input_bwd_f32(gd.data_ptr(), out.data_ptr(), n, h, w, L.stream_ptr()), 'rick_lpips_input_bwd_f32')
    ref = g[..., :3].permute(0, 3, 1, 2) / torch.tensor(SCALE, dtype=torch.float32).view(1, 3, 1, 1)
    assert torch.equal(_take(out, (n, 3, h, w)), ref)


# ---- the whole path -------------------------------------------------------------------------------------------------------
def _loss_and_grad(net, x, target):
    xr = x.clone().requires_grad_(True)
    val = net.loss(xr, target)
    g, = torch.autograd.grad(val.sum(), xr)
    return val.detach(), g


@pytest.mark.parametrize('broadcast', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_loss_and_gradient_vs_fp64(sd, net32, case, broadcast):
    x, y, vref, ref = reference(sd, case, broadcast)
    xd, yd = x.to(DEV), y.to(DEV)
    val, g = _loss_and_grad(net32, xd, yd)
    assert torch.equal(val, net32(xd, yd.expand_as(xd)))                  # the forward value is net(x, y), bit for bit
    assert torch.equal(net32.loss(xd, net32.features(yd)), val)           # no gradient wanted: the no-grad launches
    err = rel_err(g.cpu(), ref)
    print(f'LPIPS.loss at {case}, broadcast={broadcast}: gradient {err:.3e} (bound {bound(case, broadcast):.3e}), '
          f'value {float(((val.cpu().double() - vref).abs() / vref).max()):.3e}')
    assert err <= bound(case, broadcast)
    val2, g2 = _loss_and_grad(net32, xd, net32.features(yd))
    assert torch.equal(val2, val) and torch.equal(g2, g)                  # run to run
    if case[2] > 1:                                                       # image 1 alone
        v1, g1 = _loss_and_grad(net32, xd[1:2], yd if broadcast else yd[1:2])
        assert torch.equal(v1, val[1:2]) and torch.equal(g1, g[1:2])


def test_loss_upstream_gradient_and_error_cases(sd, net32):
    x, y = images(3, 16, 16, 1).to(DEV), images(3, 16, 16, 2).to(DEV)
    _, g = _loss_and_grad(net32, x, y)
    xr = x.clone().requires_grad_(True)
    gw, = torch.autograd.grad((net32.loss(xr, y) * torch.tensor([1.0, 0.0, 1.0], device=DEV)).sum(), xr)
    assert torch.equal(gw[0], g[0]) and torch.equal(gw[2], g[2]) and torch.all(gw[1] == 0)
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(net32.loss(xr, y).sum(), xr, create_graph=True)
    with pytest.raises(RuntimeError, match='quantize'):
        net32.loss(xr, y, quantize=True)
    with pytest.raises(ValueError, match='workspace'):
        net32.loss(images(4, 32, 32, 1).to(DEV).requires_grad_(True), images(4, 32, 32, 2).to(DEV))
    first = net32.loss(xr, y)
    net32.loss(xr, y)                                                     # a second forward overwrites the activations
    with pytest.raises(RuntimeError, match='overwritten'):
        torch.autograd.grad(first.sum(), xr)


def test_forward_backward_under_graph_capture(sd, net32):
    x, y = images(3, 32, 32, 3).to(DEV), images(3, 32, 32, 4).to(DEV)
    tf = net32.features(y)
    eager_val, eager_g = _loss_and_grad(net32, x, tf)
    static = torch.zeros_like(x).requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                            # warm-up on the side stream
        torch.autograd.grad(net32.loss(static, tf).sum(), static)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        val = net32.loss(static, tf)
        g, = torch.autograd.grad(val.sum(), static)
    with torch.no_grad():
        static.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(val.detach(), eager_val) and torch.equal(g, eager_g)


# ---- the projector --------------------------------------------------------------------------------------------------------
def test_projector_on_a_synthetic_generator(sd):
    from rick_amd.lpips import LPIPS
    from rick_amd.models import Generator
    from rick_amd.project import project
    from rick_amd.synth import synth_state_dict
    from tests.shapes import generator_shapes
    size = 64
    gen = Generator(size, 512, 8)
    gen.load_state_dict(synth_state_dict(generator_shapes(size)), strict=False)
    gen = gen.to(DEV)
    net = LPIPS.load(sd, device=DEV, batch=2, size=size)
    kw = dict(n_mean_latent=1000, noise=0.0)

    def run(target, steps=20):
        return project(gen, target, net, steps=steps, rng=torch.Generator().manual_seed(3), **kw)

    def G(latent):
        with torch.no_grad():
            return gen([latent], input_is_latent=True, randomize_noise=False)[0]
    # w*: one noise-free step away from the mean latent (step 0 has learning rate 0), towards some smooth image
    w_a, _, _ = run(images(1, size, size, 31), steps=2)
    w_b, _, _ = run(images(1, size, size, 32), steps=2)
    t_a, t_b = G(w_a), G(w_b)
    latent, img, losses = run(t_a)
    assert latent.shape == (1, 512) and img.shape == (1, 3, size, size) and losses.shape == (20,)
    assert bool(torch.isfinite(losses).all()) and float(losses[-1]) < float(losses[0])
    print(f'projector: loss {float(losses[0]):.5f} -> {float(losses[-1]):.5f}')
    assert torch.equal(img, G(latent))
    again = run(t_a)
    assert all(torch.equal(a, b) for a, b in zip((latent, img, losses), again))
    both, _, _ = run(torch.cat([t_a, t_b]))
    assert torch.equal(both[0:1], latent) and torch.equal(both[1:2], run(t_b)[0])
    wp, img_p, _ = project(gen, t_a, net, steps=3, w_plus=True, mse=0.1, rng=torch.Generator().manual_seed(3), **kw)
    assert wp.shape == (1, gen.n_latent, 512) and torch.equal(img_p, G(wp))
