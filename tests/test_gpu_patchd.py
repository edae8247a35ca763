"""rick_patch_head_fwd_f32 / rick_patch_head_bwd_f32 / rick_patch_head_bwd_finish_f32 and patchd.patch_head on them
(rick_amd/patchd.py, rick_amd/csrc/patchd.hip) against the literal fp64 restatement of tests/patchd_f64.py.

Every bound follows DESIGN.md section 7: four times the error that the plain fp32 torch composition (F.conv2d + leaky_relu on the
CPU) makes against the same fp64 reference on the same inputs, both over the reference's max-norm, measured here per shape (never
a constant).  Inputs are x, w ~ N(0, 1), b = 0.1.  The backward launches get an `out` equal to the fp64 reference's output rounded
to fp32, so the device and the reference take the same signs and no pixel is left out; where autograd runs end to end the
reference takes the signs of the device's own output.  The figures each test prints (run with -s) are the ones quoted in
DESIGN.md section 7."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

from tests import patchd_f64 as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SLOPE, GAIN = 0.2, 2 ** 0.5

# (N, C, H, W): only the centre tap is live; borders dominate; C is no multiple of the 64-lane group's 256 channels, odd sizes;
# more than one forward block and backward slab in both directions; across 512 channels (a second channel round forward, a third
# channel chunk backward); the two production maps; the channel cap (LDS above 64 KB forward, eight chunks backward)
SHAPES = [(1, 4, 1, 1), (2, 8, 3, 5), (3, 36, 7, 9), (2, 64, 33, 17), (1, 516, 5, 5), (2, 512, 16, 16), (4, 512, 32, 32),
          (1, 2048, 4, 4)]
_cache = {}


def _ids(s):
    return 'x'.join(map(str, s))


def _compose32(x, w, b, wscale, slope=SLOPE, gain=GAIN):
    """The plain fp32 torch composition on the CPU: the base of the fourfold rule."""
    return F.leaky_relu(F.conv2d(x, w * wscale, padding=1) + b.view(1, -1, 1, 1), slope) * gain


def _rel(a, r):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    return float(np.abs(a.reshape(r.shape) - r).max() / np.abs(r).max())


def _case(shape):
    """Inputs, the fp64 reference (forward; backward with the signs of its own output rounded to fp32) and the errors of the fp32
    composition against it — computed once per shape and shared."""
    if shape not in _cache:
        x, w, b, g, wscale = ref.case(shape)
        out64 = ref.head_fwd(x, w, b, wscale, SLOPE, GAIN)
        out_r = torch.from_numpy(out64).float()
        gx64, gw64, gb64 = ref.head_bwd(x, w, g, out_r, wscale, SLOPE, GAIN)
        base = {'out': _rel(_compose32(x, w, b, wscale), out64)}
        xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        gz32 = g * (GAIN * torch.where(out_r > 0, 1.0, SLOPE))
        z = F.conv2d(xr, wr * wscale, padding=1)
        bx, bw = torch.autograd.grad(z, (xr, wr), gz32)
        base.update(gx=_rel(bx, gx64), gw=_rel(bw, gw64), gb=_rel(gz32.sum().view(1), gb64))
        _cache[shape] = dict(x=x, w=w, b=b, g=g, wscale=wscale, out64=out64, out_r=out_r, gx64=gx64, gw64=gw64, gb64=gb64, base=base)
    return _cache[shape]


def _dev(t):
    return t.to(DEV).contiguous()


def _devx(t):
    """The feature map as the discriminator hands it over: channels-last."""
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def _bwd(x, w, g, out, wscale, slope=SLOPE, gain=GAIN, want_gx=True):
    """The two backward launches on device tensors (x channels-last), with `out` as given -> gX (logical NCHW), gw, gb."""
    from rick_amd import _lib
    N, C, H, W = x.shape
    assert x.is_contiguous(memory_format=torch.channels_last) or H * W == 1
    gx = torch.empty_like(x) if want_gx else None
    gw, gb = torch.empty_like(w), torch.empty(1, device=x.device)
    ws = torch.empty(_lib.lib.rick_patch_head_workspace_bytes(N, H, W, C) // 4, device=x.device)
    _lib.check(_lib.lib.rick_patch_head_bwd_f32(x.data_ptr(), w.data_ptr(), g.data_ptr(), out.data_ptr(), _lib.ptr(gx), ws.data_ptr(),
                                                N, H, W, C, wscale, slope, gain, _lib.stream_ptr()), 'rick_patch_head_bwd_f32')
    _lib.check(_lib.lib.rick_patch_head_bwd_finish_f32(ws.data_ptr(), gw.data_ptr(), gb.data_ptr(), N, H, W, C, wscale,
                                                       _lib.stream_ptr()), 'rick_patch_head_bwd_finish_f32')
    return gx, gw, gb


@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_head_vs_fp64(shape):
    from rick_amd import patchd
    c = _case(shape)
    x, w, b, g, out_r = _devx(c['x']), _dev(c['w']), _dev(c['b']), _dev(c['g']), _dev(c['out_r'])
    out = patchd.patch_head(x, w, b, c['wscale'])
    assert out.shape == (shape[0], 1, shape[2], shape[3]) and out.dtype == torch.float32 and out.is_contiguous()
    gx, gw, gb = _bwd(x, w, g, out_r, c['wscale'])
    assert gx.stride() == x.stride()
    gw_only = _bwd(x, w, g, out_r, c['wscale'], want_gx=False)
    assert gw_only[0] is None and torch.equal(gw_only[1], gw) and torch.equal(gw_only[2], gb)      # gx = NULL: the same sums
    for name, got, want in (('out', out, c['out64']), ('gx', gx, c['gx64']), ('gw', gw, c['gw64']), ('gb', gb, c['gb64'])):
        err, base = _rel(got, want), c['base'][name]
        print(f'patch head {_ids(shape)} {name}: device {err:.3e}  fp32 composition {base:.3e}  bound {4 * base:.3e}')
    for name, got, want in (('out', out, c['out64']), ('gx', gx, c['gx64']), ('gw', gw, c['gw64']), ('gb', gb, c['gb64'])):
        assert _rel(got, want) <= 4 * c['base'][name], name


@pytest.mark.parametrize('shape', [(3, 36, 7, 9), (2, 512, 16, 16)], ids=_ids)
def test_autograd_end_to_end_vs_fp64(shape):
    """patch_head under autograd: the reference's a takes the signs of the device's own output."""
    from rick_amd import patchd
    c = _case(shape)
    x, w, b = _devx(c['x']).requires_grad_(True), _dev(c['w']).requires_grad_(True), _dev(c['b']).requires_grad_(True)
    out = patchd.patch_head(x, w, b, c['wscale'])
    assert out.grad_fn is not None and 'PatchHeadFn' in type(out.grad_fn).__name__
    gx, gw, gb = torch.autograd.grad(out, (x, w, b), _dev(c['g']), retain_graph=True)
    assert gx.stride() == x.stride() and gw.shape == w.shape and gb.shape == b.shape
    rx, rw, rb = ref.head_bwd(c['x'], c['w'], c['g'], out.detach().cpu(), c['wscale'], SLOPE, GAIN)
    xr, wr, br = (c[k].clone().requires_grad_(True) for k in ('x', 'w', 'b'))
    bx, bw, bb = torch.autograd.grad(_compose32(xr, wr, br, c['wscale']), (xr, wr, br), c['g'])
    for name, got, base, want in (('gx', gx, bx, rx), ('gw', gw, bw, rw), ('gb', gb, bb, rb)):
        err, bs = _rel(got, want), _rel(base, want)
        print(f'patch head autograd {_ids(shape)} {name}: device {err:.3e}  fp32 composition {bs:.3e}  bound {4 * bs:.3e}')
        assert err <= 4 * bs, name
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(out.sum(), x, create_graph=True)


# ---- exact ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('q', [(0, 0), (4, 5), (0, 3), (2, 0), (2, 3)], ids=lambda q: f'{q[0]}_{q[1]}')
def test_delta_pins_taps_and_borders(q):
    """x = 1 at one (n, c0, q), b = 0, wscale = gain = slope = 1: the output is w[c0, ky, kx] at q - (ky - 1, kx - 1) and an exact
    zero elsewhere (two corners, two edges, the interior)."""
    from rick_amd import patchd
    N, C, H, W, n, c0 = 2, 8, 5, 6, 1, 5
    w = torch.randn(1, C, 3, 3, generator=torch.Generator().manual_seed(4))
    x = torch.zeros(N, C, H, W)
    x[n, c0, q[0], q[1]] = 1.0
    want = torch.zeros(N, 1, H, W)
    for ky in range(3):
        for kx in range(3):
            y, xx = q[0] - (ky - 1), q[1] - (kx - 1)
            if 0 <= y < H and 0 <= xx < W:
                want[n, 0, y, xx] = w[0, c0, ky, kx]
    out = patchd.patch_head(_devx(x), _dev(w), torch.zeros(1, device=DEV), 1.0, 1.0, 1.0)
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize('shape', [(3, 36, 7, 9), (4, 512, 16, 16)], ids=_ids)
def test_run_to_run_and_image_independence(shape):
    """Two runs give identical results; out[n] and gX[n] of the batch equal image n run alone, bit for bit."""
    from rick_amd import patchd
    x, w, b, g, wscale = ref.case(shape, seed=17)
    x, w, b, g = _devx(x), _dev(w), _dev(b), _dev(g)
    out = patchd.patch_head(x, w, b, wscale)
    gx, gw, gb = _bwd(x, w, g, out, wscale)
    out2 = patchd.patch_head(x, w, b, wscale)
    gx2, gw2, gb2 = _bwd(x, w, g, out, wscale)
    assert torch.equal(out, out2) and torch.equal(gx, gx2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)
    for n in range(shape[0]):
        xn = x[n:n + 1].clone(memory_format=torch.channels_last)
        on = patchd.patch_head(xn, w, b, wscale)
        assert torch.equal(on, out[n:n + 1])
        gxn, _, _ = _bwd(xn, w, g[n:n + 1].clone(), on, wscale)
        assert torch.equal(gxn, gx[n:n + 1])
    # a view into the batch: another address (a 16-byte multiple: C % 4 == 0), the same values
    assert torch.equal(patchd.patch_head(x[1:2], w, b, wscale), out[1:2])


def test_gx_is_exactly_zero_for_a_zero_channel():
    shape = (3, 36, 7, 9)
    x, w, b, g, wscale = ref.case(shape, seed=23)
    w[0, 5] = 0
    w[0, 32] = 0
    from rick_amd import patchd
    x, w, b, g = _devx(x), _dev(w), _dev(b), _dev(g)
    gx, _, _ = _bwd(x, w, g, patchd.patch_head(x, w, b, wscale), wscale)
    assert not gx[:, 5].any() and not gx[:, 32].any() and gx[:, 4].any() and gx[:, 33].any()


# ---- dispatch -------------------------------------------------------------------------------------------------------------------
def _grads(fn, c):
    x, w, b = _devx(c['x']).requires_grad_(True), _dev(c['w']).requires_grad_(True), _dev(c['b']).requires_grad_(True)
    out = fn(x, w, b, c['wscale'])
    return (out,) + torch.autograd.grad(out, (x, w, b), _dev(c['g']))


_paths = {}


@pytest.mark.parametrize('name', ['out', 'gx', 'gw', 'gb'])
def test_kernel_and_composed_paths_agree(name):
    """(2, 512, 16, 16): the kernels and the composition of the existing ops (op.conv2d + fused_leaky_relu), each through autograd
    with the signs of its own output, agree within the sum of their two fourfold bounds, 4 base + 4 base, over the reference's
    max-norm.

    Measured on MI355X (difference / bound; composed and kernels against fp64): out 2.7e-7 / 1.7e-6 (2.0e-7, 1.4e-7), gX 3.1e-7 /
    1.2e-6 (2.8e-7, 1.5e-7), gw 1.8e-7 / 5.6e-6 (1.8e-7, 7.8e-8), gb 1.1e-7 / 3.3e-7 (6.9e-8, 4.2e-8).  The gb case is why the
    composition adds the bias in fp64 before fused_leaky_relu (patchd._compose): with the bias handed to fused_leaky_relu the
    difference was 3.1e-6, that op's fp32 block-partial column sum over the 512 values of the one channel."""
    from rick_amd import patchd
    c = _case((2, 512, 16, 16))
    if not _paths:
        _paths['kernels'] = _grads(patchd.patch_head, c)
        assert patchd.use_kernels(False) is True
        try:
            _paths['composed'] = _grads(patchd.patch_head, c)
        finally:
            patchd.use_kernels(True)
        assert 'PatchHeadFn' in type(_paths['kernels'][0].grad_fn).__name__
        assert 'PatchHeadFn' not in type(_paths['composed'][0].grad_fn).__name__
    k = ('out', 'gx', 'gw', 'gb').index(name)
    a, b, want = _paths['kernels'][k], _paths['composed'][k], c[name + '64']
    diff = float((a.detach().double() - b.detach().double()).abs().max().cpu() / np.abs(want).max())
    bound = 4 * c['base'][name] + 4 * c['base'][name]
    print(f'kernels vs composed {name}: difference {diff:.3e}  (composed vs fp64 {_rel(b, want):.3e}, kernels {_rel(a, want):.3e})  '
          f'bound {bound:.3e}')
    assert diff <= bound


def test_ineligible_shape_takes_the_composition():
    """C = 6: silently the composition of the existing ops, within their documented 2e-6 of fp64 (tests/test_gpu_ops.py)."""
    from rick_amd import patchd
    shape = (2, 6, 5, 7)
    x, w, b, g, wscale = ref.case(shape)
    xd, wd, bd = _devx(x).requires_grad_(True), _dev(w).requires_grad_(True), _dev(b).requires_grad_(True)
    out = patchd.patch_head(xd, wd, bd, wscale)
    assert 'PatchHeadFn' not in type(out.grad_fn).__name__
    gx, gw, gb = torch.autograd.grad(out, (xd, wd, bd), _dev(g))
    assert _rel(out, ref.head_fwd(x, w, b, wscale, SLOPE, GAIN)) <= 2e-6
    rx, rw, rb = ref.head_bwd(x, w, g, out.detach().cpu(), wscale, SLOPE, GAIN)
    assert _rel(gx, rx) <= 2e-6 and _rel(gw, rw) <= 2e-6 and _rel(gb, rb) <= 2e-6


# ---- teacher-forced, on the discriminator's own tap -----------------------------------------------------------------------------
@pytest.mark.parametrize('p_ind', [0, 1, 2])
def test_teacher_forced_tap_gradient(p_ind):
    """32-px discriminator, batch 2: the tap feature the device trunk produced goes through head, loss and the gradient with
    respect to that feature in fp64 on the CPU (the signs of the device's own patch map); the device's gradient at the tap
    (retain_grad) is held to four times the fp32 composition's error."""
    from rick_amd import patchd
    from rick_amd.models import Discriminator
    from rick_amd.train import d_logistic_loss
    torch.manual_seed(11)
    d, heads = Discriminator(32).to(DEV), patchd.PatchHeads(n_heads=3).to(DEV)
    img = torch.randn(2, 3, 32, 32, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    seen = {}
    inner = heads.forward

    def tapped(x, p):
        x.retain_grad()
        seen['tap'], seen['out'] = x, inner(x, p)
        return seen['out']
    heads.forward = tapped
    pred = patchd.patch_logits(d, heads, img, p_ind)
    fake, real = pred.chunk(2, 0)
    d_logistic_loss(real, fake).backward()
    tap, conv, act = seen['tap'], heads.new_conv[p_ind][0], heads.new_conv[p_ind][1]
    assert tap.shape[1] == 512 and tap.shape[2] in (32, 16) and 'PatchHeadFn' in type(seen['out'].grad_fn).__name__
    x, w, b = tap.detach().cpu(), conv.weight.detach().cpu(), act.bias.detach().cpu()
    o64 = torch.from_numpy(ref.head_fwd(x, w, b, conv.scale, SLOPE, GAIN)).requires_grad_(True)
    f64, r64 = o64.chunk(2, 0)
    (g64,) = torch.autograd.grad(d_logistic_loss(r64, f64), o64)
    want, _, _ = ref.head_bwd(x, w, g64, pred.detach().cpu(), conv.scale, SLOPE, GAIN)
    x32 = x.clone().requires_grad_(True)
    f32, r32 = _compose32(x32, w, b, conv.scale).chunk(2, 0)
    (base,) = torch.autograd.grad(d_logistic_loss(r32, f32), x32)
    err, bs = _rel(tap.grad, want), _rel(base, want)
    print(f'teacher-forced tap {p_ind} {tuple(tap.shape)}: device {err:.3e}  fp32 composition {bs:.3e}  bound {4 * bs:.3e}')
    assert err <= 4 * bs
    # nothing behind the exit block got a gradient
    exit_blk = 1 if p_ind < 2 else 2
    for n, p in d.named_parameters():
        behind = (n.startswith('final') or int(n.split('.')[1]) > exit_blk
                  or (p_ind != 1 and n.startswith(f'convs.{exit_blk}.') and 'conv1' not in n))      # a t1 tap: conv1 only
        assert (p.grad is None) == behind, n
