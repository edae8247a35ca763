"""GPU: the VGG16 fc2 kernels (rick_amd/csrc/vgg.hip) against exact and fp64 references, the whole network against the
independent fp64 restatement (tests/vgg_f64.py), batch invariance, graph capture, and the evaluator's precision / recall end
to end.  The conftest's autouse fixture asserts after every test that the saturation counter stayed at 0.

Tolerances.  The f32-input MFMA forms exact fp32 products, so the device differs from an fp32 CPU computation by the order of
its fp32 sums only (K <= 25088).  For every comparison the base figure is the error of the fp32 torch CPU composition
against the same fp64 reference on the same inputs (max error over the reference's max-norm, measured once on the CPU and
written down below); the device bound is that figure x 4, which covers a different blocking of the same sums."""
import pytest
import torch
import torch.nn.functional as F

from tests.vgg_f64 import SmoothG, fc2_f64_batched, max_rel_err, pr_margin, smooth_images, synthetic_vgg16_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0
SIZES = [256, 224, 299, 64, 200]

# fp32 torch CPU F.linear (+ ReLU) against fp64 on fc_inputs(M, K, N): (without ReLU, with ReLU)
FC_CPU_BASE = {
    (1, 512, 64): (1.246e-07, 1.089e-07),
    (3, 1000, 200): (1.839e-07, 1.678e-07),
    (3, 1003, 200): (1.325e-07, 1.325e-07),                  # K not a multiple of 4: scalar x loads, zero-padded k tail
    (25, 25088, 4096): (3.693e-07, 3.901e-07),
    (50, 4096, 4096): (4.284e-07, 4.614e-07),
    (64, 25088, 4096): (3.332e-07, 3.265e-07),
}
# fp32 torch CPU network (VGG16Fc2Features on CPU tensors) against the fp64 restatement on network_inputs(size)[:n], keyed (size, n)
NET_CPU_BASE = {(64, 3): 8.551e-07, (64, 27): 8.583e-07, (256, 3): 9.710e-07, (256, 27): 9.955e-07}
FACTOR = 4


def _lib():
    from rick_amd import _lib
    return _lib


# ---- input kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(s, s) for s in SIZES] + [(100, 317)])
def test_input_kernel_is_the_cpu_index_rule(hw):
    from rick_amd.vgg import resize_nearest
    L = _lib()
    h, w = hw
    x = torch.randn(2, 3, h, w, generator=torch.Generator().manual_seed(h))
    out = torch.full((2, 224, 224, 4), SENTINEL, device=DEV)
    L.check(L.lib.rick_vgg_input_f32(x.to(DEV).data_ptr(), out.data_ptr(), 2, h, w, L.stream_ptr()), 'rick_vgg_input_f32')
    got = out.cpu()
    assert torch.equal(got[..., :3], resize_nearest(x).permute(0, 2, 3, 1))
    assert torch.equal(got[..., :3], F.interpolate(x, size=(224, 224)).permute(0, 2, 3, 1))
    assert torch.all(got[..., 3] == 0)


# ---- fc kernel ------------------------------------------------------------------------------------------------------------
_FC_CACHE = {}


def fc_inputs(M, K, N):
    """x [M, K] (the first M of 64 seeded rows), W [N, K] with std sqrt(2 / K), bias [N]; one (W, bias, x) per (K, N)."""
    if (K, N) not in _FC_CACHE:
        _FC_CACHE.clear()                                    # one fc1-sized weight (411 MB) at a time
        g = torch.Generator().manual_seed(K * 7 + N)
        _FC_CACHE[(K, N)] = (torch.randn(64, K, generator=g), torch.randn(N, K, generator=g) * (2.0 / K) ** 0.5,
                             torch.randn(N, generator=g) * 0.1)
    x, w, b = _FC_CACHE[(K, N)]
    return x[:M].contiguous(), w, b


def fc_reference(x, w, b, relu):
    y = F.linear(x.double(), w.double(), b.double())
    return torch.relu(y) if relu else y


class _Fc:
    """One packed layer on the device."""

    def __init__(self, w, b):
        from rick_amd.vgg import pack_fc_weight
        L = _lib()
        self.n, self.k = w.shape
        wpk = pack_fc_weight(w)
        assert wpk.numel() == L.lib.rick_fc_packed_floats(self.k, self.n)
        self.wpk, self.b = wpk.to(DEV), b.to(DEV)

    def __call__(self, x, relu):
        L = _lib()
        m = x.shape[0]
        floats = L.lib.rick_fc_workspace_floats(m, self.k, self.n)
        assert floats >= m * self.n
        ws = torch.full((floats + 64,), SENTINEL, device=DEV)                 # 64 guard floats behind the workspace
        out = torch.full((m + 1, self.n), SENTINEL, device=DEV)               # one guard row behind the output
        L.check(L.lib.rick_fc_f32(x.data_ptr(), self.wpk.data_ptr(), self.b.data_ptr(), ws.data_ptr(), out.data_ptr(), m, self.k,
                                  self.n, int(relu), L.stream_ptr()), 'rick_fc_f32')
        assert torch.all(ws[floats:] == SENTINEL) and torch.all(out[m] == SENTINEL)
        return out[:m]


@pytest.mark.parametrize('M,K,N', list(FC_CPU_BASE))
def test_fc_kernel_vs_fp64(M, K, N):
    x, w, b = fc_inputs(M, K, N)
    fc = _Fc(w, b)
    xd = x.to(DEV)
    for relu in (False, True):
        ref = fc_reference(x, w, b, relu)
        got = fc(xd, relu)
        again = fc(xd, relu)
        err = max_rel_err(got.cpu(), ref)
        base = FC_CPU_BASE[(M, K, N)][int(relu)]
        print(f'rick_fc_f32 M={M} K={K} N={N} relu={int(relu)}: max err / max-norm {err:.3e} '
              f'(fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
        assert torch.equal(got, again)                                        # run to run
        assert err <= FACTOR * base
        if relu:
            assert float(got.min()) == 0.0


def test_fc_rows_do_not_depend_on_m_or_on_other_rows():
    x, w, b = fc_inputs(64, 25088, 4096)
    fc = _Fc(w, b)
    xd = x.to(DEV)
    full = fc(xd, False)
    assert torch.equal(fc(xd[:25].contiguous(), False), full[:25])
    for m in (0, 24, 40, 63):
        assert torch.equal(fc(xd[m:m + 1].contiguous(), False), full[m:m + 1])
    # row 40 next to different rows
    other = torch.randn(25, 25088, generator=torch.Generator().manual_seed(5)).to(DEV)
    other[7] = xd[40]
    assert torch.equal(fc(other, False)[7], full[40])


def test_fc_x_alignment_and_k_tail_do_not_change_the_sums():
    """x that is not 16-byte aligned takes the scalar load path: the same values in the same order, so the same bits.  A K
    that is no multiple of 8 ends in a zero-padded k block: appending zero columns to x and W up to the next multiple of 8
    adds exact zeros at the end of the chain."""
    x, w, b = fc_inputs(3, 1000, 200)
    fc = _Fc(w, b)
    aligned = fc(x.to(DEV), True)
    shifted = torch.full((x.numel() + 1,), SENTINEL, device=DEV)[1:]          # 4 bytes past a 16-byte boundary
    assert shifted.data_ptr() % 16 == 4
    shifted.copy_(x.to(DEV).view(-1))
    assert torch.equal(fc(shifted.view(3, 1000), True), aligned)
    x, w, b = fc_inputs(3, 1003, 200)
    tail = _Fc(w, b)(x.to(DEV), False)
    padded = _Fc(F.pad(w, (0, 5)), b)(F.pad(x, (0, 5)).to(DEV), False)        # K = 1008: vector loads, no tail
    assert torch.equal(tail, padded)


def test_fc_rejects_what_it_does_not_support():
    L = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    p = t.data_ptr()
    for m in (0, 65):
        assert L.lib.rick_fc_f32(p, p, p, p, p, m, 64, 64, 0, L.stream_ptr()) == 22
        assert L.lib.rick_fc_workspace_floats(m, 64, 64) < 0
    assert L.lib.rick_fc_f32(None, p, p, p, p, 1, 64, 64, 0, L.stream_ptr()) == 22


# ---- whole network --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def sd():
    return synthetic_vgg16_state_dict(0)


@pytest.fixture(scope='module')
def net(sd):
    from rick_amd.vgg import VGG16Fc2Features
    return VGG16Fc2Features.load(sd, device=DEV, batch=25)


_NET_REF = {}


def network_inputs(size):
    return smooth_images(27, size, seed=size + 1)


def _network_reference(sd, size):
    if size not in _NET_REF:
        _NET_REF[size] = fc2_f64_batched(sd, network_inputs(size))
    return _NET_REF[size]


@pytest.mark.parametrize('size', [64, 256])
@pytest.mark.parametrize('n', [3, 27])
def test_network_vs_fp64(sd, net, size, n):
    x = network_inputs(size)[:n]
    ref = _network_reference(sd, size)[:n]
    got = net(x.to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 4096) and got.device.type == 'cuda'
    err = max_rel_err(got.cpu(), ref)
    base = NET_CPU_BASE[(size, n)]
    print(f'fc2 features at {size}^2, n={n}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.equal(net(x.to(DEV)), got)


@pytest.mark.parametrize('size', [64, 256])
def test_features_do_not_depend_on_the_batch(net, size):
    x = network_inputs(size).to(DEV)
    full = net(x)                                             # chunks of 25 + 2
    assert torch.equal(net(x[:3]), full[:3])
    assert torch.equal(net(x[24:27]), full[24:27])            # image 24: last of a chunk there, first of one here
    assert torch.equal(net(x[26:27]), full[26:27])
    assert torch.equal(net(x.flip(0)).flip(0), full)


def test_graph_capture_replays_the_eager_result(net):
    x = network_inputs(64)[:5].to(DEV)
    eager = net(x)
    static = x.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net(static)                                           # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = net(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(network_inputs(64)[5:10])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, net(network_inputs(64)[5:10].to(DEV)))


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_evaluator_precision_recall_vs_fp64(sd, net):
    from rick_amd.evaluate import Evaluator, precision_recall_from_features
    n_real, n_fake, size, k = 14, 12, 32, 3
    g = SmoothG(size).to(DEV)
    z = torch.randn(n_fake, 512, generator=torch.Generator().manual_seed(39))
    real = smooth_images(n_real, size, seed=40, low=4) * 0.9
    with torch.no_grad():
        fake = g([z.to(DEV)])[0].cpu()
    fr64, ff64 = fc2_f64_batched(sd, real), fc2_f64_batched(sd, fake)
    margin = pr_margin(fr64, ff64, k)
    print(f'precision / recall margin of the sample set: {margin:.2e}')
    assert margin > 1e-4                                      # the condition under which fp32 features cannot flip a count
    p_ref, r_ref = (float(v) for v in precision_recall_from_features(fr64, ff64, k=k))
    assert 0 < p_ref + r_ref < 2
    inception = lambda img: F.adaptive_avg_pool2d(img, 4).flatten(1)          # noqa: E731  (stands in for Inception pool3)
    ev = Evaluator(g, inception, inception(real.to(DEV)), n_sample_store=6, inception_nsamples=n_fake, fid_sample_size=n_fake,
                   pr_feature_fn=net, real_pr_feats=net(real.to(DEV)), k=k)
    got = ev.compute_inception_score(fid=False, pr=True, latents=z)
    assert got['precision'].device.type == 'cuda'
    # The counts are compared, not the quotients: count / n is an fp64 division on whichever device holds the features,
    # and the device's division may differ from the host's in the last bit (5 / 12 does).  A count is an integer, so
    # share * n is within 1e-9 of it on either side and a flipped count moves it by 1.
    counts = lambda p, r: (p * n_fake, r * n_real)                            # noqa: E731
    hits_ref = tuple(round(v) for v in counts(p_ref, r_ref))
    assert all(abs(v - h) < 1e-9 for v, h in zip(counts(p_ref, r_ref), hits_ref))
    hits = counts(float(got['precision']), float(got['recall']))
    print(f'covered fake / real samples: {hits} (fp64 restatement {hits_ref})')
    assert all(abs(v - h) < 1e-9 for v, h in zip(hits, hits_ref))
