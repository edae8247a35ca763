"""GPU: the LPIPS kernels (rick_amd/csrc/lpips.hip) against exact and fp64 references, the whole network against the
independent fp64 restatement (tests/lpips_f64.py), batch invariance, determinism next to a busy process, and intra_lpips
end to end against an fp64 oracle."""
import ctypes
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests.lpips_f64 import lpips_f64, lpips_matrix_f64, smooth_images, synthetic_state_dict, to_unit
from tests.test_lpips import roundtrip_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0


def _lib():
    from rick_amd import _lib
    return _lib


@pytest.fixture(scope='module')
def sd():
    return synthetic_state_dict(0)


@pytest.fixture(scope='module')
def net64(sd):
    from rick_amd.lpips import LPIPS
    return LPIPS.load(sd, device=DEV, batch=50, size=64)


def _input(x, mode, u8out=None):
    L = _lib()
    n, _, h, w = x.shape
    out = torch.full((n, h, w, 4), SENTINEL, device=DEV)
    xf, xq = (None, x.data_ptr()) if mode == 2 else (x.data_ptr(), None)
    L.check(L.lib.rick_lpips_input_f32(xf, xq, out.data_ptr(), None if u8out is None else u8out.data_ptr(), n, h, w, mode,
                                       L.stream_ptr()), 'rick_lpips_input_f32')
    return out.cpu()


def test_input_kernel_is_bit_exact():
    from rick_amd.lpips import scale_input
    q = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).repeat(2, 3, 1, 1)
    q[1] = q[1].flip(-1)
    got = _input(q.to(DEV), 2)
    ref, _ = scale_input(q)
    assert torch.equal(got[..., :3], ref.permute(0, 2, 3, 1)) and torch.all(got[..., 3] == 0)
    # floats, round trip off
    x = torch.rand(2, 3, 17, 23, generator=torch.Generator().manual_seed(0)) * 2.2 - 1.1
    ref, _ = scale_input(x)
    assert torch.equal(_input(x.to(DEV), 0)[..., :3], ref.permute(0, 2, 3, 1))
    # floats through the PNG round trip: every uint8 threshold +- 8 float32 steps, on every channel
    xs = torch.from_numpy(roundtrip_inputs())
    x = xs.view(1, 1, 1, -1).repeat(1, 3, 1, 1)
    x[0, 1] = x[0, 1].flip(-1)
    u8 = torch.zeros(x.shape, dtype=torch.uint8, device=DEV)
    ref, qref = scale_input(x, quantize=True)
    assert torch.equal(_input(x.to(DEV), 1, u8)[..., :3], ref.permute(0, 2, 3, 1))
    assert torch.equal(u8.cpu(), qref)


@pytest.mark.parametrize('hw', [(16, 16), (17, 23), (33, 9), (2, 3)])
def test_maxpool2_matches_torch(hw):
    L = _lib()
    x = torch.randn(3, 64, *hw, generator=torch.Generator().manual_seed(hw[0]))
    xn = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    oh, ow = hw[0] // 2, hw[1] // 2
    out = torch.full((3, oh, ow, 64), SENTINEL, device=DEV)
    L.check(L.lib.rick_lpips_maxpool2_f32(xn.data_ptr(), out.data_ptr(), 3, hw[0], hw[1], 64, L.stream_ptr()),
            'rick_lpips_maxpool2_f32')
    assert torch.equal(out.cpu(), F.max_pool2d(x, 2, 2).permute(0, 2, 3, 1))


@pytest.mark.parametrize('C', [64, 128, 512, 260])
def test_inverse_norm(C):
    L = _lib()
    f = torch.relu(torch.randn(7, 13, C, generator=torch.Generator().manual_seed(C)))
    f[2, 5] = 0
    f[6] = 0
    out = torch.full((7 * 13,), SENTINEL, device=DEV)
    L.check(L.lib.rick_lpips_invnorm_f32(f.to(DEV).data_ptr(), out.data_ptr(), 7 * 13, C, L.stream_ptr()), 'rick_lpips_invnorm_f32')
    got = out.cpu().view(7, 13)
    s = f.double().pow(2).sum(-1)
    ref = torch.where(s > 0, 1 / (s.sqrt() + 1e-10), torch.zeros_like(s))
    assert got[2, 5] == 0 and torch.all(got[6] == 0) and torch.isfinite(got).all()
    ok = s > 0
    assert float(((got.double() - ref).abs()[ok] / ref[ok]).max()) <= 1e-6


def _random_features(n, size, seed):
    from rick_amd.lpips import LpipsFeatures
    g = torch.Generator().manual_seed(seed)
    f = LpipsFeatures.empty(n, size, size, 'cpu')
    taps = [torch.relu(torch.randn(t.shape, generator=g)) for t in f.taps]
    inorm = [torch.rand(t.shape, generator=g) + 0.5 for t in f.inorm]
    return LpipsFeatures([t.to(DEV) for t in taps], [t.to(DEV) for t in inorm])


def _direct_f64(net, fa, fb):
    out = torch.zeros(fa.n, fb.n, dtype=torch.float64)
    for s in range(5):
        a = (fa.taps[s].cpu().double() * fa.inorm[s].cpu().double().view(fa.taps[s].shape[:3])[..., None]).flatten(1, 2)
        b = (fb.taps[s].cpu().double() * fb.inorm[s].cpu().double().view(fb.taps[s].shape[:3])[..., None]).flatten(1, 2)
        w = net.lins[s].double()
        for i in range(fa.n):
            out[i] += ((a[i:i + 1] - b) ** 2 * w).sum(2).mean(1)
    return out


def test_pair_kernel_vs_fp64_and_exact_properties(net64):
    fa, fb = _random_features(19, 32, 1), _random_features(21, 32, 2)
    D = net64.distances(fa, fb)
    ref = _direct_f64(net64, fa, fb)
    err = float(((D.double().cpu() - ref).abs() / ref).max())
    print(f'pair kernel max rel err vs fp64: {err:.2e}')
    assert err <= 1e-6
    assert torch.equal(net64.distances(fb, fa), D.t())                      # D(A, B) == D(B, A)^T bitwise
    Daa = net64.distances(fa, fa)
    assert torch.all(torch.diagonal(Daa) == 0) and torch.equal(Daa, Daa.t())
    # a sub-block of a larger call, alone
    sub = net64.distances(fa.narrow(5, 12), fb.narrow(17, 19))
    assert torch.equal(sub, D[5:12, 17:19])
    one = net64.distances(fa.narrow(18, 19), fb.narrow(0, 1))
    assert torch.equal(one, D[18:19, 0:1])


@pytest.mark.parametrize('size,n', [(64, 4), (256, 2)])
def test_network_vs_fp64(sd, size, n):
    from rick_amd.lpips import LPIPS
    net = LPIPS.load(sd, device=DEV, batch=4, size=size)
    x, y = smooth_images(n, size, seed=5), smooth_images(n, size, seed=6)
    ref = lpips_f64(sd, x, y)
    got = net(x.to(DEV), y.to(DEV)).double().cpu()
    err = float(((got - ref).abs() / ref).max())
    Dref = lpips_matrix_f64(sd, x, y)
    D = net.distances(net.features(x.to(DEV)), net.features(y.to(DEV))).double().cpu()
    errD = float(((D - Dref).abs() / Dref).max())
    print(f'LPIPS at {size}^2: paired max rel err {err:.2e}, matrix {errD:.2e} (values {ref.min():.3f} .. {ref.max():.3f})')
    assert err <= 1e-4 and errD <= 1e-4
    # through the uint8 round trip: the same as feeding the quantised images
    q = ((x / 2 + 0.5) * 255 + 0.5).clamp(0, 255).to(torch.uint8)
    fq, fu = net.features(x.to(DEV), quantize=True), net.features(q.to(DEV))
    assert all(torch.equal(a, b) for a, b in zip(fq.taps + fq.inorm, fu.taps + fu.inorm))


def test_batch_invariance(net64):
    x = smooth_images(50, 64, seed=7).to(DEV)
    y = smooth_images(3, 64, seed=8).to(DEV)
    fy = net64.features(y)
    whole = net64.features(x)
    D = net64.distances(whole, fy)
    for step in (1, 7):
        for lo in range(0, 50, step):
            part = net64.features(x[lo:lo + step])
            for a, b in zip(part.taps + part.inorm, whole.narrow(lo, lo + step).taps + whole.narrow(lo, lo + step).inorm):
                assert torch.equal(a, b), (step, lo)
            assert torch.equal(net64.distances(part, fy), D[lo:lo + step])


def test_repeated_calls_are_bitwise_equal_next_to_a_busy_neighbour(net64):
    x, y = smooth_images(9, 64, seed=9).to(DEV), smooth_images(9, 64, seed=10).to(DEV)
    d0 = net64.distances(net64.features(x), net64.features(y))
    p0 = net64(x, y)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    agg = subprocess.Popen([sys.executable, os.path.join(root, 'tools', 'stress_ops.py'), '--role', 'aggressor', '--seconds', '120'],
                           stdout=subprocess.PIPE, text=True)
    differing = 0
    try:
        for line in agg.stdout:
            if 'ready' in line:
                break
        assert agg.poll() is None, 'the neighbour process died before it started'
        for _ in range(20):
            differing += int(not torch.equal(net64.distances(net64.features(x), net64.features(y)), d0))
            differing += int(not torch.equal(net64(x, y), p0))
        torch.cuda.synchronize()
        assert agg.poll() is None, 'the neighbour process ended before the measurement did'
    finally:
        agg.kill() if agg.poll() is None else None
        agg.wait()
    assert differing == 0


class _SmoothG(torch.nn.Module):
    """A generator stand-in on the device: bilinear upsampling of tanh(z) seen as 3 x 4 x 4 (smooth, distinct images)."""

    def __init__(self, size):
        super().__init__()
        self.size = size
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, zs):
        z = zs[0]
        img = torch.tanh(z[:, :48]).view(-1, 3, 4, 4)
        return F.interpolate(img, (self.size, self.size), mode='bilinear', align_corners=False) * 0.9, None


def _oracle_check(sd, net, g, centers, n_samples, n_store, cluster_size, seed, size):
    from rick_amd.evaluate import assign_clusters, cluster_subsets, intra_lpips
    latents = torch.randn(n_samples + n_store, 512, generator=torch.Generator().manual_seed(seed))
    val, per, counts = intra_lpips(g, centers, net, n_samples=n_samples, n_sample_store=n_store, cluster_size=cluster_size,
                                   size=size, latents=latents, rng=torch.Generator().manual_seed(seed))
    n = int(counts.sum())
    with torch.no_grad():
        imgs = torch.cat([g([latents[i:i + n_store].to(DEV)])[0] for i in range(0, n, n_store)])[:n]
    q = ((imgs / 2 + 0.5) * 255 + 0.5).clamp(0, 255).to(torch.uint8).cpu()
    dc = lpips_matrix_f64(sd, to_unit(q), to_unit(centers))
    # the device's assignment (its features are batch-invariant, so these are the distances intra_lpips used)
    dev_assign = assign_clusters(net.distances(net.features(q.to(DEV)), net.features(centers.to(DEV))))
    top2 = dc.topk(2, dim=1, largest=False).values
    sure = (top2[:, 1] - top2[:, 0]) > 1e-4
    assert torch.equal(dev_assign[sure], dc.argmin(1)[sure])
    assert torch.equal(counts, torch.bincount(dev_assign, minlength=centers.shape[0]))
    subsets = cluster_subsets(dev_assign, centers.shape[0], cluster_size, torch.Generator().manual_seed(seed))
    ref = torch.full((centers.shape[0],), math.nan, dtype=torch.float64)
    for c, idx in enumerate(subsets):
        if idx.numel() >= 2:
            x = to_unit(q[idx])
            d = lpips_matrix_f64(sd, x, x)
            ref[c] = d[torch.triu(torch.ones(len(idx), len(idx), dtype=torch.bool), 1)].mean()
    assert torch.equal(torch.isnan(per), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    assert int(ok.sum()) >= 2
    err = float(((per[ok] - ref[ok]).abs() / ref[ok]).max())
    err_v = abs(val - float(ref[ok].mean())) / float(ref[ok].mean())
    print(f'intra_lpips at {size}^2: {n} samples, counts {counts.tolist()}, value {val:.6f}, '
          f'per-cluster max rel err {err:.2e}, value rel err {err_v:.2e}')
    assert err <= 1e-5 and err_v <= 1e-5


def test_intra_lpips_vs_fp64_oracle_64px(sd, net64):
    centers = ((smooth_images(4, 64, seed=12, low=4) * 0.9 / 2 + 0.5) * 255).to(torch.uint8)
    _oracle_check(sd, net64, _SmoothG(64).to(DEV), centers, 60, 25, 8, 13, 64)


def test_intra_lpips_vs_fp64_oracle_256px(sd):
    from rick_amd.lpips import LPIPS
    net = LPIPS.load(sd, device=DEV, batch=6)
    centers = ((smooth_images(2, 256, seed=14, low=4) * 0.9 / 2 + 0.5) * 255).to(torch.uint8)
    _oracle_check(sd, net, _SmoothG(256).to(DEV), centers, 12, 6, 50, 15, 256)


def test_defaults_stay_within_the_memory_bound(sd):
    from rick_amd.evaluate import intra_lpips
    from rick_amd.lpips import LPIPS
    g = _SmoothG(256).to(DEV)
    centers = ((smooth_images(10, 256, seed=16, low=4) * 0.9 / 2 + 0.5) * 255).to(torch.uint8)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    net = LPIPS.load(sd, device=DEV, batch=25)
    val, per, counts = intra_lpips(g, centers, net, rng=torch.Generator().manual_seed(0))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f'intra_lpips defaults: value {val:.4f}, counts {counts.tolist()}, peak {peak / 2**30:.2f} GiB above the generator')
    assert int(counts.sum()) == 1000 and math.isfinite(val)
    assert peak <= 8 * 2**30
