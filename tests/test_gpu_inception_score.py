"""GPU: the Inception Score kernels (rick_amd/csrc/inception.hip: rick_inc_input_raw_f32, rick_is_rows_f32,
rick_is_accum_f64) against exact and fp64 references, and the whole path (InceptionV3Logits, InceptionScoreStats, Evaluator)
against the fp64 restatement (tests/inception_score_f64.py) at the smallest sizes.  The conftest's autouse fixture asserts
after every test that the saturation counter stayed at 0.

Tolerances.  The f32-input MFMA forms exact fp32 products, so the device differs from an fp32 CPU computation by the order of
its fp32 sums only.  The base figure of a comparison is the error of the fp32 torch CPU composition against the same fp64
reference on the same inputs (tests/test_inception_score.py: CPU_BASE, measured once on the CPU), the device bound is that
figure x 4.  The fp64 kernels are held to an fp64 torch loop directly: the accumulation bit for bit, the rows' s and h within
the rounding of their own fp64 operations; the rows' fp32 softmax is held to 4 x the error of torch's fp32 CPU softmax (its
expf) on the same rows (ROWS_CPU_BASE)."""
import pytest
import torch
import torch.nn.functional as F

from tests.inception_score_f64 import score_f64, smooth_images
from tests.test_inception_score import CPU_BASE, FACTOR, case, max_rel

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0


def _lib():
    from rick_amd import _lib
    return _lib


# ---- input kernels ----------------------------------------------------------------------------------------------------------
def _input(entry, x, oh, ow):
    L = _lib()
    n, _, h, w = x.shape
    out = torch.full((n + 1, oh, ow, 4), SENTINEL, device=DEV)               # one guard image behind the output
    L.check(getattr(L.lib, entry)(x.to(DEV).contiguous().data_ptr(), out.data_ptr(), n, h, w, oh, ow, L.stream_ptr()), entry)
    got = out.cpu()
    assert torch.all(got[n] == SENTINEL) and torch.all(got[:n, ..., 3] == 0)
    return got[:n, ..., :3].permute(0, 3, 1, 2)


@pytest.mark.parametrize('hw', [(75, 75), (80, 96)])
def test_raw_input_is_a_bit_exact_copy_at_the_native_size(hw):
    x = torch.randn(3, 3, *hw, generator=torch.Generator().manual_seed(hw[1]))
    x[0, 0, 0, :4] = torch.tensor([-0.0, 0.0, 1e-42, -3e38])                 # signed zero, a denormal, a large value
    got = _input('rick_inc_input_raw_f32', x, *hw)
    assert torch.equal(got.view(torch.int32), x.view(torch.int32))


@pytest.mark.parametrize('hw', [(64, 64), (80, 96)])
def test_raw_input_resize_vs_fp64(hw):
    x = torch.rand(3, 3, *hw, generator=torch.Generator().manual_seed(hw[0])) * 2 - 1
    got = _input('rick_inc_input_raw_f32', x, 299, 299)
    ref = F.interpolate(x.double(), (299, 299), mode='bilinear', align_corners=False)
    # fp32 source coordinates (as torch's own fp32 kernel computes them): the bound of tests/test_gpu_inception.py
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4


@pytest.mark.parametrize('hw', [(64, 64), (80, 96), (299, 299)])
def test_feature_extractor_input_keeps_its_affine(hw):
    from rick_amd.inception import MEAN, STD
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[0] + 1)) * 2 - 1
    got = _input('rick_inc_input_f32', x, 299, 299)
    r = F.interpolate(x.double(), (299, 299), mode='bilinear', align_corners=False)
    ref = torch.stack([r[:, c] * (STD[c] / 0.5) + (MEAN[c] - 0.5) / 0.5 for c in range(3)], 1)
    assert float((got.double() - ref).abs().max() / ref.abs().max()) < 1e-4   # test_input_kernel_vs_fp64's bound


# ---- rows kernel ------------------------------------------------------------------------------------------------------------
# torch's fp32 CPU softmax against the fp64 softmax on rows_input(64, C): the largest over the rows of max |d| over the row's
# max-norm (rows_err).  Rows are independent, so the figure of the 64 rows bounds that of their first 1 or 5.
ROWS_CPU_BASE = {1: 0.0, 7: 1.602e-07, 64: 1.326e-07, 65: 1.733e-07, 1000: 4.279e-07}


def rows_err(p, ref):
    return float(((p.double() - ref).abs().max(1).values / ref.abs().max(1).values).max())


def rows_input(M, C):
    """The first M of 64 seeded rows of logits with a standard deviation of 3; row 1 has one logit 200 above the rest, row 2
    is constant."""
    z = torch.randn(64, C, generator=torch.Generator().manual_seed(C)) * 3
    z[1, C // 2] = z[1].max() + 200
    z[2] = 1.25
    return z[:M].contiguous()


def _rows(z):
    L = _lib()
    M, C = z.shape
    zd = z.to(DEV)
    p = torch.full((M + 1, C), SENTINEL, device=DEV)
    s = torch.full((M + 1,), SENTINEL, device=DEV, dtype=torch.float64)
    h = torch.full((M + 1,), SENTINEL, device=DEV, dtype=torch.float64)
    L.check(L.lib.rick_is_rows_f32(zd.data_ptr(), p.data_ptr(), s.data_ptr(), h.data_ptr(), M, C, L.stream_ptr()),
            'rick_is_rows_f32')
    assert torch.all(p[M] == SENTINEL) and float(s[M]) == SENTINEL and float(h[M]) == SENTINEL
    return p[:M].cpu(), s[:M].cpu(), h[:M].cpu()


def _check_rows(z):
    M, C = z.shape
    p, s, h = _rows(z)
    p2, s2, h2 = _rows(z)
    assert torch.equal(p, p2) and torch.equal(s, s2) and torch.equal(h, h2)   # run to run
    ref = torch.softmax(z.double(), -1)
    err = rows_err(p, ref)
    base = ROWS_CPU_BASE[C]
    print(f'rick_is_rows_f32 M={M} C={C}: p max err / row max-norm {err:.3e} (fp32 CPU softmax {base:.3e}, '
          f'bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    # s and h against the fp64 expressions on the kernel's own p: C additions, and per term a division, a log and a product
    pd = p.double()
    s_ref = pd.sum(1)
    assert float(((s - s_ref).abs() / s_ref).max()) <= 2 * C * 2.0 ** -53     # either side's C - 1 additions
    q = pd / s[:, None]
    terms = torch.xlogy(q, q)
    slack = 2 * (C + 3) * 2.0 ** -53 * terms.abs().sum(1)
    assert bool(torch.isfinite(h).all()) and bool(((h - terms.sum(1)).abs() <= slack).all()), (h - terms.sum(1)).abs().max()
    return p, s, h


@pytest.mark.parametrize('C', [1, 7, 64, 65, 1000])
@pytest.mark.parametrize('M', [1, 5, 64])
def test_rows_kernel_vs_fp64(M, C):
    z = rows_input(M, C)
    p, s, h = _check_rows(z)
    if M >= 5 and C > 1:
        assert float(p[1, C // 2]) == 1.0 and int((p[1] == 0).sum()) == C - 1 and float(h[1]) == 0.0      # exact zeros
        assert torch.equal(p[2], torch.full((C,), 1.0, dtype=torch.float32) / C)                          # p = 1 / C


@pytest.mark.parametrize('C', [1, 7, 64, 65, 1000])
def test_rows_kernel_single_special_rows(C):
    """The spike row and the constant row as calls of one row (M = 1 holds only the random row above)."""
    z = rows_input(5, C)
    p, _, h = _check_rows(z[1:2].contiguous())
    if C > 1:
        assert float(p[0, C // 2]) == 1.0 and int((p[0] == 0).sum()) == C - 1
    assert float(h[0]) == 0.0
    p, s, h = _check_rows(z[2:3].contiguous())
    assert torch.equal(p[0], torch.full((C,), 1.0, dtype=torch.float32) / C)
    if C > 1:
        log_c = float(torch.log(torch.tensor(float(C), dtype=torch.float64)))
        assert abs(float(h[0]) + log_c) <= 2 * (C + 3) * 2.0 ** -53 * log_c     # sum q = 1 and log q = -log C to rounding


def test_rows_and_accumulate_reject_bad_arguments():
    L = _lib()
    t = torch.zeros(64, device=DEV, dtype=torch.float64)
    p = t.data_ptr()
    assert L.lib.rick_is_rows_f32(p, p, p, p, 1, 0, L.stream_ptr()) == 22
    assert L.lib.rick_is_rows_f32(None, p, p, p, 1, 4, L.stream_ptr()) == 22
    assert L.lib.rick_is_accum_f64(p, p, p, p, 1, 4, 0, 0, 1, L.stream_ptr()) == 22
    assert L.lib.rick_is_accum_f64(p, p, p, p, 1, 4, 1, 0, 0, L.stream_ptr()) == 22
    assert L.lib.rick_is_accum_f64(p, p, p, p, 1, 4, 1, -1, 1, L.stream_ptr()) == 22
    assert L.lib.rick_inc_input_raw_f32(p, None, 1, 8, 8, 8, 8, L.stream_ptr()) == 22


# ---- accumulate kernel ------------------------------------------------------------------------------------------------------
def test_accumulate_is_bit_identical_however_the_rows_are_cut():
    from rick_amd.inception import accumulate_rows, softmax_rows
    M, C, S, per = 10, 1000, 3, 3
    z = rows_input(M, C).to(DEV)
    p, s, h = softmax_rows(z)

    def run(cuts, rows=M):
        acc = torch.zeros(S + 1, 2 * C + 1, device=DEV, dtype=torch.float64)     # one guard split behind the state
        acc[S] = SENTINEL
        lo = 0
        for m in cuts:
            accumulate_rows(acc[:S], p[lo:lo + m].contiguous(), s[lo:lo + m].contiguous(), h[lo:lo + m].contiguous(), lo, per)
            lo += m
        assert lo == rows and torch.all(acc[S] == SENTINEL)
        return acc[:S].cpu()

    whole = run([10])
    assert torch.equal(run([4, 6]), whole) and torch.equal(run([1] * 10), whole)
    assert torch.equal(run([9], rows=9), whole)                                  # row 9 = 3 * 3 is dropped
    pc, sc, hc = p.cpu().double(), s.cpu(), h.cpu()
    ref = torch.zeros(S, 2 * C + 1, dtype=torch.float64)
    for g in range(S * per):                                                     # the kernel's order: ascending rows
        k = g // per
        ref[k, :C] += pc[g]
        ref[k, C:2 * C] += pc[g] / sc[g]
        ref[k, 2 * C] += hc[g]
    assert torch.equal(whole, ref)


# ---- whole path -------------------------------------------------------------------------------------------------------------
_NETS = {}
# rows_err of torch's fp32 CPU softmax on the 70 x 1000 fp64 logits of 'native75n70' rounded to fp32 (the largest of the cases)
ROWS_CPU_BASE_NET = 2.787e-07


def _net(name, batch=8):
    from rick_amd.inception import InceptionV3Logits
    if (name, batch) not in _NETS:
        _, size, sd, _ = case(name)
        _NETS[(name, batch)] = InceptionV3Logits.load(sd, device=DEV, batch=batch, size=size)
    return _NETS[(name, batch)]


@pytest.mark.parametrize('name,batch', [('native75', 8), ('native80x96', 8), ('resize64', 8), ('native75n70', 100)])
def test_logits_and_score_vs_fp64(name, batch):
    from rick_amd.evaluate import inception_score
    images, size, sd, ref = case(name)
    net = _net(name, batch)                           # batch 100 at N = 70: one plan run, the fc in chunks of 64 + 6 rows
    x = images.to(DEV)
    got = net(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (images.shape[0], 1000) and got.is_cuda
    base, sbase = CPU_BASE[name]
    err = max_rel(got, ref)
    print(f'{name}: logits max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.equal(net(x), got)                                              # run to run
    assert torch.equal(net(x[1:2]), got[1:2])                                    # a row does not depend on N
    assert torch.equal(net(x[-1:]), got[-1:])
    p = net.probs(x)
    assert rows_err(p.cpu(), torch.softmax(got.double().cpu(), -1)) <= FACTOR * ROWS_CPU_BASE_NET
    for splits in (1, 2):
        want = score_f64(ref, splits)
        mean, std = inception_score(x, net, splits)
        assert mean.is_cuda and mean.dtype == torch.float64 and std.dtype == torch.float64
        rel = abs(float(mean) - want[0]) / want[0]
        print(f'{name}: score splits {splits}: {float(mean):.6f} (fp64 {want[0]:.6f}) rel {rel:.3e} '
              f'(fp32 CPU {sbase:.3e}, bound {FACTOR * sbase:.3e}); std {float(std):.6f} (fp64 {want[1]:.6f})')
        assert rel <= FACTOR * sbase
        assert abs(float(std) - want[1]) <= FACTOR * sbase * (want[0] + want[1])     # the larger split score
        again = inception_score(x, net, splits)
        assert torch.equal(again[0], mean) and torch.equal(again[1], std)


def test_score_does_not_depend_on_the_batches():
    from rick_amd.evaluate import InceptionScoreStats
    images = case('native75n70')[0].to(DEV)
    net = _net('native75n70', 100)
    whole = InceptionScoreStats(net, 70, 2).update(images)
    parts = InceptionScoreStats(net, 70, 2)
    for lo, hi in ((0, 8), (8, 9), (9, 64), (64, 70)):
        parts.update(images[lo:hi])
    assert torch.equal(parts.acc, whole.acc)
    a, b = parts.finalize(), whole.finalize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_graph_replay_equals_eager():
    net = _net('native75')
    a, b = smooth_images(4, 75, 75, 21).to(DEV), smooth_images(4, 75, 75, 22).to(DEV)
    eager_a, eager_b = net(a), net(b)
    static = a.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net(static)                                                              # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = net(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    static.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b)


def test_wrong_size_and_device_are_errors():
    net = _net('native75')
    with pytest.raises(RuntimeError, match='75, 75'):
        net(torch.zeros(1, 3, 80, 80, device=DEV))
    assert tuple(net(torch.zeros(2, 3, 75, 75)).shape) == (2, 1000)              # CPU tensors: the torch composition


def test_evaluator_equals_hand_called_statistics_bitwise():
    from rick_amd.evaluate import Evaluator, InceptionScoreStats
    from rick_amd.models import Generator
    from rick_amd.synth import synth_latents, synth_state_dict
    from tests.shapes import generator_shapes
    g = Generator(64, 512, 8, channel_multiplier=2)
    g.load_state_dict(synth_state_dict(generator_shapes(64)), strict=False)
    g = g.to(DEV).eval()
    fwd = g.forward
    g.forward = lambda styles, **kw: fwd(styles, randomize_noise=False, **kw)
    net = _net('resize64')                                                       # 64 px images, resized to 299
    z = synth_latents(12, seed=15).to(DEV)
    feature_fn = lambda img: F.adaptive_avg_pool2d(img, 2).flatten(1)            # noqa: E731  (stands in for pool3)
    real = feature_fn(smooth_images(12, 64, 64, 16).to(DEV))
    ev = Evaluator(g, feature_fn, real, n_sample_store=5, inception_nsamples=12, fid_sample_size=11, is_net=net)
    got = ev.compute_inception_score(fid=True, latents=z, iscore=True, is_splits=2)
    assert set(got) == {'fid', 'is', 'is_std'} and got['is'].is_cuda
    st = InceptionScoreStats(net, 11, 2)
    with torch.no_grad():
        for lo, take in ((0, 5), (5, 5), (10, 1)):                               # the first 11 of the 12 generated images
            st.update(g([z[lo:lo + 5]])[0][:take])
    mean, std = st.finalize()
    assert torch.equal(got['is'], mean) and torch.equal(got['is_std'], std)
    assert bool(torch.isfinite(mean)) and float(mean) >= 1.0
    assert set(ev.compute_inception_score(fid=True, latents=z)) == {'fid'}
