"""GPU: the perceptual path length (rick_amd/ppl.py) — rick_ppl_latents_f32 and rick_lpips_paired_f32 against fp64 and against
the kernels they must agree with bit for bit, the routing of LPIPS.__call__ / LPIPS.loss through the paired kernel, and the
metric end to end against the fp64 restatement (tests/ppl_f64.py).

"The fp32 torch composition" below is tests/ppl_f64.py (or the expression written out in the test) evaluated in float32 on the
CPU; its own deviation from the float64 evaluation of the same inputs is the yardstick, never the code under test."""
import ctypes
import functools

import pytest
import torch

from rick_amd.synth import synth_state_dict
from tests import ppl_f64
from tests.lpips_f64 import smooth_images, synthetic_state_dict
from tests.shapes import generator_shapes

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0
EINVAL = 22


def _lib():
    from rick_amd import _lib
    return _lib


# ---- rick_ppl_latents_f32 -------------------------------------------------------------------------------------------------
def _latent_case(B, L, eps, seed):
    """a, b [B, L], t [B]: t cycles through 0, 0.5, 1 - eps and random values; from B = 3 on row 1 has b == a and row 2 has b
    nearly parallel to a (1e-3 of noise on 1.7 a: acos works at d = 1 - 2e-7, three fp32 steps below 1)."""
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)
    t = torch.rand(B, generator=g)
    fixed = [0.5] if B == 1 else [0.0, 0.5, 1.0 - eps]
    for i in range(B):
        if i % 4 < len(fixed):
            t[i] = fixed[i % 4]
    if B >= 3:
        b[1] = a[1]
        b[2] = a[2] * 1.7 + 1e-3 * torch.randn(L, generator=g)
    return a, b, t


def _launch(a, b, t, eps, mode):
    """The kernel on device copies of a, b, t -> out [2B, L] on the CPU; one guard row behind the output must stay untouched."""
    L = _lib()
    B, n = a.shape
    out = torch.full((2 * B + 1, n), SENTINEL, device=DEV)
    da, db, dt = a.to(DEV), b.to(DEV), t.to(DEV)                      # named: the buffers must outlive the launch
    rc = L.lib.rick_ppl_latents_f32(da.data_ptr(), db.data_ptr(), dt.data_ptr(), eps, out.data_ptr(), B, n, mode, L.stream_ptr())
    assert rc == 0, rc
    out = out.cpu()
    assert torch.all(out[2 * B] == SENTINEL) and not torch.any(out[:2 * B] == SENTINEL)
    return out[:2 * B]


def _errors(x, ref):
    """(max abs element error, max abs error of row 2i + 1 - row 2i relative to the max-norm of its fp64 value)."""
    x = x.double()
    dref = ref[1::2] - ref[0::2]
    return float((x - ref).abs().max()), float(((x[1::2] - x[0::2]) - dref).abs().max() / dref.abs().max())


@pytest.mark.parametrize('eps', [1e-4, 1e-2])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('L', [5, 64, 512, 1000])
@pytest.mark.parametrize('B', [1, 3, 8])
def test_latents_kernel_vs_fp64(B, L, mode, eps):
    """Per element, and for the difference of a pair's two rows, the error against fp64 is at most 2 x the fp32 torch
    composition's (only the order of the sums differs from it; in fact the kernel computes in fp64 and rounds once).  Observed
    on an MI355X host over the 48 cases: largest ratio 1.27 per element (B = 8, L = 64, w, eps 1e-4) and 1.46 for the pair
    difference (B = 3, L = 5, z, eps 1e-4: 1.20e-04 against 8.21e-05) -- two independently rounded fp32 rows differ by up to
    one ulp, while the composition's two rows share part of their rounding.  The yardstick is the host CPU's fp32 result and
    moves with its libm: with another host's the same kernel output gave up to 1.80 (B = 3, L = 512, z, eps 1e-4)."""
    space = 'wz'[mode]
    a, b, t = _latent_case(B, L, eps, 100 * B + L)
    ref = ppl_f64.path_latents(a, b, t, eps, space)
    yard = _errors(ppl_f64.path_latents(a, b, t, eps, space, dtype=torch.float32), ref)
    got = _launch(a, b, t, eps, mode)
    assert torch.isfinite(got).all()
    err = _errors(got, ref)
    print(f'latents B={B} L={L} {space} eps={eps:g}: element err {err[0]:.2e} (fp32 composition {yard[0]:.2e}), '
          f'pair difference rel err {err[1]:.2e} ({yard[1]:.2e})')
    assert err[0] <= 2 * yard[0] and err[1] <= 2 * yard[1]
    if mode == 1:
        assert float((got.double().norm(dim=1) - 1).abs().max()) <= 2e-7
    from rick_amd.ppl import path_latents
    assert torch.equal(path_latents(a.to(DEV), b.to(DEV), t.to(DEV), eps, space).cpu(), got)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('L', [5, 512, 1000])
def test_latents_kernel_is_batch_invariant_and_repeatable(L, mode):
    a, b, t = _latent_case(8, L, 1e-4, L)
    whole = _launch(a, b, t, 1e-4, mode)
    assert torch.equal(_launch(a, b, t, 1e-4, mode), whole)
    for i in range(8):
        assert torch.equal(_launch(a[i:i + 1], b[i:i + 1], t[i:i + 1], 1e-4, mode), whole[2 * i:2 * i + 2]), i


def test_latents_kernel_refuses_bad_arguments():
    L = _lib()
    a, b, t = (x.to(DEV) for x in _latent_case(2, 16, 1e-4, 0))
    out = torch.full((4, 16), SENTINEL, device=DEV)
    ok = dict(a=a.data_ptr(), b=b.data_ptr(), t=t.data_ptr(), eps=1e-4, out=out.data_ptr(), B=2, L=16, mode=0)
    bads = [dict(a=None), dict(b=None), dict(t=None), dict(out=None), dict(eps=0.0), dict(eps=-1e-4), dict(eps=float('inf')),
            dict(eps=float('nan')), dict(mode=2), dict(mode=-1), dict(L=0), dict(L=1025), dict(B=-1)]
    for bad in bads:
        kw = dict(ok)
        kw.update(bad)
        assert L.lib.rick_ppl_latents_f32(kw['a'], kw['b'], kw['t'], kw['eps'], kw['out'], kw['B'], kw['L'], kw['mode'],
                                          L.stream_ptr()) == EINVAL, bad
    torch.cuda.synchronize()
    assert torch.all(out == SENTINEL)
    from rick_amd.ppl import path_latents
    with pytest.raises(ValueError, match=r'ppl\.path_latents'):
        path_latents(torch.zeros(1, 1028, device=DEV), torch.zeros(1, 1028, device=DEV), torch.zeros(1, device=DEV), 1e-4, 'z')


# ---- rick_lpips_paired_f32 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sd():
    return synthetic_state_dict(0)


@pytest.fixture(scope='module')
def net64(sd):
    from rick_amd.lpips import LPIPS
    return LPIPS.load(sd, device=DEV, batch=12, size=64)


def _random_features(n, h, w, seed):
    """As tests/test_gpu_lpips.py: ReLU'd normal taps, inverse norms in [0.5, 1.5) (CPU)."""
    from rick_amd.lpips import LpipsFeatures
    g = torch.Generator().manual_seed(seed)
    f = LpipsFeatures.empty(n, h, w, 'cpu')
    return LpipsFeatures([torch.relu(torch.randn(t.shape, generator=g)) for t in f.taps],
                         [torch.rand(t.shape, generator=g) + 0.5 for t in f.inorm])


def _to(f, dev):
    from rick_amd.lpips import LpipsFeatures
    return LpipsFeatures([t.to(dev).contiguous() for t in f.taps], [t.to(dev).contiguous() for t in f.inorm])


def _rows(f, k):
    from rick_amd.lpips import LpipsFeatures
    return LpipsFeatures([t[k::2].contiguous() for t in f.taps], [t[k::2].contiguous() for t in f.inorm])


def _paired_direct(net, fa, fb, dtype):
    """sum over taps of mean over positions of sum_c w_c (a ia - b ib)^2 for image i against image i, in ``dtype`` (CPU)."""
    out = 0
    for s in range(5):
        a = (fa.taps[s].to(dtype) * fa.inorm[s].to(dtype).view(fa.taps[s].shape[:3])[..., None]).flatten(1, 2)
        b = (fb.taps[s].to(dtype) * fb.inorm[s].to(dtype).view(fb.taps[s].shape[:3])[..., None]).flatten(1, 2)
        out = out + ((a - b) ** 2 * net.lins[s].to(dtype)).sum(2).mean(1)
    return out


@pytest.mark.parametrize('n', [1, 2, 5])
@pytest.mark.parametrize('hw', [(16, 16), (17, 23), (64, 64)])
def test_paired_kernel_is_the_diagonal_of_the_pair_kernel(net64, hw, n):
    inter = _random_features(2 * n, *hw, seed=hw[0] + n)
    fa, fb = _to(_rows(inter, 0), DEV), _to(_rows(inter, 1), DEV)
    got = net64.paired(fa, fb)
    assert got.shape == (n,) and torch.equal(got, torch.diagonal(net64.distances(fa, fb)))
    assert torch.equal(net64.paired(_to(inter, DEV)), got)                    # one interleaved set, image stride 2
    assert torch.equal(net64.paired(fb, fa), got)                              # (a - b)^2 is symmetric, bit for bit
    ref = _paired_direct(net64, _rows(inter, 0), _rows(inter, 1), torch.float64)
    err = float(((got.double().cpu() - ref).abs() / ref).max())
    print(f'paired kernel {hw} n={n}: max rel err vs fp64 {err:.2e}')
    assert err <= 1e-6
    assert torch.all(net64.paired(fa, fa) == 0)


def test_paired_kernel_on_near_pairs(net64):
    """y = x + 1e-4 noise, where a Gram form would cancel: the direct form's relative error against fp64 is bounded by 4 x the
    fp32 torch composition's on the same pairs.  Measured on an MI355X: 1.79e-06 for the kernel and 1.79e-06 for the fp32
    composition (values 7.7e-07 .. 8.4e-07): both are the rounding of a ia and b ib ahead of a difference 1e-4 of their size."""
    fa = _random_features(3, 64, 64, seed=7)
    g = torch.Generator().manual_seed(8)
    from rick_amd.lpips import LpipsFeatures
    fb = LpipsFeatures([t + 1e-4 * torch.randn(t.shape, generator=g) for t in fa.taps], [t.clone() for t in fa.inorm])
    ref = _paired_direct(net64, fa, fb, torch.float64)
    yard = float(((_paired_direct(net64, fa, fb, torch.float32).double() - ref).abs() / ref).max())
    got = net64.paired(_to(fa, DEV), _to(fb, DEV))
    assert torch.equal(got, torch.diagonal(net64.distances(_to(fa, DEV), _to(fb, DEV))))
    err = float(((got.double().cpu() - ref).abs() / ref).max())
    print(f'paired kernel, near pairs: rel err vs fp64 {err:.2e}, fp32 composition {yard:.2e} (values {ref.min():.3e} .. {ref.max():.3e})')
    assert yard > 0 and err <= 4 * yard


def test_paired_entry_refuses_bad_arguments(net64):
    L = _lib()
    f = _to(_random_features(2, 16, 16, seed=1), DEV)
    part = torch.full((8,), SENTINEL, device=DEV, dtype=torch.float64)
    ta, ia, w = f.taps[0].data_ptr(), f.inorm[0].data_ptr(), net64._plan.lins[0].data_ptr()
    ok = [ta, ia, 1, ta, ia, 1, 2, w, 256, 64, 128, part.data_ptr()]
    for pos, bad in ((0, None), (1, None), (3, None), (4, None), (7, None), (11, None), (2, 0), (5, 0), (6, -1), (8, 0), (9, 62),
                     (9, 2048), (10, 0), (10, 256), (0, ta + 4)):
        args = list(ok)
        args[pos] = bad
        assert L.lib.rick_lpips_paired_f32(*args, L.stream_ptr()) == EINVAL, (pos, bad)
    torch.cuda.synchronize()
    assert torch.all(part == SENTINEL)


@pytest.mark.parametrize('hw', [(64, 64), (48, 40)])
def test_call_and_loss_run_on_the_paired_kernel_with_the_same_bits(net64, hw):
    """net(x, y) and the no-grad net.loss(x, y) equal the diagonal of the all-pairs route, at the planned size and off it."""
    g = torch.Generator().manual_seed(hw[1])
    x = smooth_images(3, 64, seed=21)[:, :, :hw[0], :hw[1]].contiguous().to(DEV)
    y = (x + 0.05 * torch.randn(x.shape, generator=g).to(DEV)).clamp(-1, 1)
    want = torch.diagonal(net64.distances(net64.features(x), net64.features(y))).contiguous()
    assert bool((want > 0).all())
    assert torch.equal(net64(x, y), want)
    with torch.no_grad():
        assert torch.equal(net64.loss(x, y), want)
    assert torch.equal(net64.loss(x, net64.features(y)), want)
    assert torch.equal(net64.loss(x.clone().requires_grad_(), y).detach(), want)


# ---- the metric end to end ------------------------------------------------------------------------------------------------
SIZE, N, EPS = 32, 6, 1e-2


@pytest.fixture(scope='module')
def world():
    from rick_amd.lpips import LPIPS
    from rick_amd.models import Generator
    sg = synth_state_dict(generator_shapes(SIZE, n_mlp=2, cm=1))
    sl = synthetic_state_dict(3)
    g = Generator(SIZE, 512, 2, channel_multiplier=1)
    g.load_state_dict(sg, strict=False)
    return sg, sl, g.to(DEV).eval(), LPIPS.load(sl, device=DEV, batch=8, size=SIZE)


@functools.lru_cache(maxsize=None)
def _reference(space, crop):
    """fp64 distances of the pinned paths and the fp32 composition's relative deviation from them, once per (space, crop)."""
    sg, sl = synth_state_dict(generator_shapes(SIZE, n_mlp=2, cm=1)), synthetic_state_dict(3)
    latents, noise = ppl_f64.pinned_paths(N, SIZE, 11)
    ref = ppl_f64.path_distances(sg, sl, SIZE, *latents, noise, EPS, space, crop)
    f32 = ppl_f64.path_distances(sg, sl, SIZE, *latents, noise, EPS, space, crop, dtype=torch.float32)
    return ref, float(((f32.double() - ref).abs() / ref).max())


def _saturation_count():
    c = ctypes.c_uint(0)
    _lib().check(_lib().lib.rick_saturation_count(ctypes.byref(c), 0), 'rick_saturation_count')
    return c.value


@pytest.mark.parametrize('crop', [False, True])
@pytest.mark.parametrize('space', ['w', 'z'])
@pytest.mark.parametrize('batch', [2, 4])
def test_metric_end_to_end(world, batch, space, crop):
    """6 pinned paths on the 32 px generator, eps = 1e-2.  (i) the distances are those of the public pieces composed by hand;
    (ii) against the fp64 restatement the relative error is at most 8 x the CPU fp32 composition's (the generator's split-fp16
    convolutions: up to ~5 x fp32 rounding of the image, README); (iii) the filtered mean is the restatement's filter of the
    device's own distances, exactly; (iv) no saturation event.  Observed on an MI355X (profiles/ppl_bench.txt has the batch-4
    rows): device error 1.6e-05 .. 5.8e-05 against 4.3e-05 .. 8.8e-05 for the CPU fp32 composition, ratio 0.25 .. 1.27 over the
    eight cases (largest: space w, crop, batch 4)."""
    from rick_amd.ppl import path_latents, perceptual_path_length
    sg, sl, g, net = world
    latents, noise = ppl_f64.pinned_paths(N, SIZE, 11)
    ppl, d = perceptual_path_length(g, net, n_samples=N, batch=batch, eps=EPS, space=space, sampling='full', crop=crop,
                                    latents=latents, noise=noise)
    assert d.shape == (N,) and d.is_cuda and not g.training
    # (i)
    hand = []
    with torch.no_grad():
        for lo in range(0, N, batch):
            a, b, t = (x[lo:lo + batch].to(DEV) for x in latents)
            maps = [m[lo:lo + batch].to(DEV).repeat_interleave(2, 0) for m in noise]
            if space == 'w':
                img, _ = g([path_latents(g.get_latent(a), g.get_latent(b), t, EPS, 'w')], input_is_latent=True, noise=maps)
            else:
                img, _ = g([path_latents(a, b, t, EPS, 'z')], noise=maps)
            if crop:
                img = img[:, :, 12:28, 8:24]
            f = net.features(img.contiguous())
            hand.append(torch.diagonal(net.distances(f, f)[0::2, 1::2]) / (EPS * EPS))
    assert torch.equal(d, torch.cat(hand))
    # (ii)
    ref, yard = _reference(space, crop)
    err = float(((d.double().cpu() - ref).abs() / ref).max())
    print(f'ppl end to end {space} crop={crop} batch={batch}: rel err vs fp64 {err:.2e}, CPU fp32 composition {yard:.2e}, '
          f'ratio {err / yard:.2f}')
    assert err <= 8 * yard
    # (iii), (iv)
    assert ppl == ppl_f64.filtered_mean(d.tolist())
    torch.cuda.synchronize()
    assert _saturation_count() == 0


def test_evaluator_compute_ppl(world):
    from rick_amd.evaluate import Evaluator
    from rick_amd.ppl import perceptual_path_length
    _, _, g, net = world
    latents, noise = ppl_f64.pinned_paths(N, SIZE, 12, sampling='end')
    kw = dict(n_samples=N, batch=3, eps=EPS, space='z', sampling='end', latents=latents, noise=noise)
    ev = Evaluator(g, None, None)
    want = perceptual_path_length(g, net, **kw)[0]
    assert ev.compute_ppl(net, **kw) == want and want > 0
    # drawn latents and noise: reproducible from the generator's seed, on the default 'w' / 'end' route
    a = perceptual_path_length(g, net, n_samples=5, batch=4, eps=EPS, generator=torch.Generator().manual_seed(5))
    b = perceptual_path_length(g, net, n_samples=5, batch=4, eps=EPS, generator=torch.Generator().manual_seed(5))
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and a[0] > 0
