"""CPU: the LPIPS loader (both layouts), the CPU network against the fp64 restatement (tests/lpips_f64.py), the uint8 round
trip, the intra-cluster logic of rick_amd.evaluate with stubbed distances, and load_cluster_centers."""
import math
import os

import numpy as np
import pytest
import torch

from tests.lpips_f64 import lpips_f64, lpips_matrix_f64, smooth_images, synthetic_state_dict


def _vgg_layout(sd):
    """lpips layout -> (torchvision vgg16 state_dict, lin weights file)."""
    vgg = {}
    for k, v in sd.items():
        if k.startswith('net.slice'):
            idx, p = k.split('.')[2:]
            vgg[f'features.{idx}.{p}'] = v
    vgg['classifier.0.weight'] = torch.zeros(4, 8)
    vgg['classifier.0.bias'] = torch.zeros(4)
    lin = {k: v for k, v in sd.items() if k.startswith('lin') and not k.startswith('lins.')}
    return vgg, lin


@pytest.fixture(scope='module')
def sd():
    return synthetic_state_dict(0)


def test_both_layouts_load_the_same_network(sd):
    from rick_amd.lpips import LPIPS
    a = LPIPS.load(sd, device='cpu')
    vgg, lin = _vgg_layout(sd)
    b = LPIPS.load(vgg=vgg, lin=lin, device='cpu')
    assert a.convs.keys() == b.convs.keys()
    for k in a.convs:
        assert torch.equal(a.convs[k][0], b.convs[k][0]) and torch.equal(a.convs[k][1], b.convs[k][1])
    for x, y in zip(a.lins, b.lins):
        assert torch.equal(x, y)
    # without the optional duplicates and buffers
    lean = {k: v for k, v in sd.items() if not k.startswith(('lins.', 'scaling_layer.'))}
    LPIPS.load(lean, device='cpu')


def test_loader_names_missing_and_unknown_keys(sd):
    from rick_amd.lpips import LPIPS
    bad = dict(sd)
    del bad['net.slice3.12.bias']
    with pytest.raises(KeyError, match='net.slice3.12.bias'):
        LPIPS.load(bad, device='cpu')
    bad = dict(sd)
    del bad['lin4.model.1.weight']
    with pytest.raises(KeyError, match='lin4.model.1.weight'):
        LPIPS.load(bad, device='cpu')
    bad = dict(sd, **{'net.slice5.30.weight': torch.zeros(1)})
    with pytest.raises(KeyError, match='net.slice5.30.weight'):
        LPIPS.load(bad, device='cpu')
    vgg, lin = _vgg_layout(sd)
    with pytest.raises(KeyError, match='features.30.weight'):
        LPIPS.load(vgg=dict(vgg, **{'features.30.weight': torch.zeros(1)}), lin=lin, device='cpu')
    with pytest.raises(KeyError, match='features.0.weight'):
        LPIPS.load(vgg={k: v for k, v in vgg.items() if k != 'features.0.weight'}, lin=lin, device='cpu')
    with pytest.raises(KeyError, match='lin9.model.1.weight'):
        LPIPS.load(vgg=vgg, lin=dict(lin, **{'lin9.model.1.weight': torch.zeros(1)}), device='cpu')
    with pytest.raises(ValueError, match='scaling_layer.shift'):
        LPIPS.load(dict(sd, **{'scaling_layer.shift': torch.zeros(1, 3, 1, 1)}), device='cpu')
    with pytest.raises(ValueError):
        LPIPS.load(sd, vgg=vgg, lin=lin, device='cpu')


@pytest.mark.parametrize('size', [32, 64])
@pytest.mark.parametrize('mixed', [False, True])
def test_cpu_path_vs_fp64(size, mixed):
    from rick_amd.lpips import LPIPS
    sd = synthetic_state_dict(1, mixed_sign=mixed)
    net = LPIPS.load(sd, device='cpu')
    x, y = smooth_images(3, size, seed=2), smooth_images(3, size, seed=3)
    ref = lpips_f64(sd, x, y)
    assert float(ref.min()) > 0.01, ref
    got = net(x, y)
    assert got.dtype == torch.float32 and got.shape == (3,)
    assert float(((got.double() - ref).abs() / ref.abs()).max()) <= 1e-5
    # features + distances: the same numbers as the paired call, and every pair of the matrix
    D = net.distances(net.features(x), net.features(y))
    Dref = lpips_matrix_f64(sd, x, y)
    assert float(((D.double() - Dref).abs() / Dref.abs()).max()) <= 1e-5


def _roundtrip_np(x):
    """The reference's PNG round trip + Normalize, as single float32 numpy operations (independent of torch)."""
    x = x.astype(np.float32)
    s = (x / np.float32(2) + np.float32(0.5)) * np.float32(255) + np.float32(0.5)
    q = np.clip(s, np.float32(0), np.float32(255)).astype(np.uint8)
    t = q.astype(np.float32) / np.float32(255)
    return q, (t - np.float32(0.5)) / np.float32(0.5)


def roundtrip_inputs():
    """Every uint8 threshold of the round trip, +-8 float32 steps around it, and the range ends."""
    qs = np.arange(257, dtype=np.float64)
    edges = ((qs - 0.5) / 255 - 0.5) * 2                  # x where (x / 2 + 0.5) * 255 + 0.5 crosses an integer
    xs = [np.float32(e) for e in edges]
    out = []
    for x in xs:
        v = x
        for _ in range(8):
            v = np.nextafter(v, np.float32(-2))
        for _ in range(17):
            out.append(v)
            v = np.nextafter(v, np.float32(2))
    out += [np.float32(v) for v in (-1.5, -1, 0, 1, 1.5)]
    return np.array(out, dtype=np.float32)


def test_uint8_round_trip_is_bit_exact():
    from rick_amd.lpips import SCALE, SHIFT, scale_input
    xs = roundtrip_inputs()
    n = len(xs)
    x = torch.from_numpy(np.tile(xs, 3).reshape(1, 3, 1, n))
    got, q = scale_input(x, quantize=True)
    q_ref, t_ref = _roundtrip_np(np.tile(xs, 3).reshape(1, 3, 1, n))
    assert np.array_equal(q.numpy(), q_ref)
    assert len(np.unique(q_ref)) == 256                         # every uint8 value is reached
    ref = (t_ref - np.array(SHIFT, np.float32).reshape(1, 3, 1, 1)) / np.array(SCALE, np.float32).reshape(1, 3, 1, 1)
    assert np.array_equal(got.numpy(), ref.astype(np.float32))
    got8, _ = scale_input(torch.from_numpy(q_ref))
    assert torch.equal(got8, got)


# ---- intra-cluster logic ----------------------------------------------------------------------------------------------------
def test_sample_count_rule():
    from rick_amd.evaluate import lpips_sample_count
    assert lpips_sample_count(1000, 25, 5000) == 1000
    assert lpips_sample_count(1000, 30, 5000) == 1020
    assert lpips_sample_count(1000, 30, 1010) == 1010
    assert lpips_sample_count(60, 7, 5000) == 63


def test_argmin_ties_go_to_the_lowest_index():
    from rick_amd.evaluate import assign_clusters
    d = torch.tensor([[0.3, 0.1, 0.1, 0.2], [0.5, 0.5, 0.5, 0.5], [0.2, 0.9, 0.0, 0.0], [0.4, 0.3, 0.2, 0.1]])
    assert assign_clusters(d).tolist() == [1, 0, 2, 3]


def test_subset_selection_is_reproducible_and_matches_a_restatement():
    from rick_amd.evaluate import cluster_subsets
    g = torch.Generator().manual_seed(0)
    assign = torch.randint(0, 4, (300,), generator=g)
    assign[assign == 3] = 2                                       # cluster 3 empty
    a = cluster_subsets(assign, 5, 20, rng=torch.Generator().manual_seed(7))
    b = cluster_subsets(assign, 5, 20, rng=torch.Generator().manual_seed(7))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    rng = torch.Generator().manual_seed(7)
    for c in range(5):
        members = [i for i, v in enumerate(assign.tolist()) if v == c]
        if len(members) > 20:
            perm = torch.randperm(len(members), generator=rng)[:20].tolist()
            members = [members[p] for p in perm]
        assert a[c].tolist() == members
    assert [len(s) for s in a] == [20, 20, 20, 0, 0]


def test_nan_clusters_are_excluded_and_all_nan_is_nan():
    from rick_amd.evaluate import mean_pair_distance, nan_mean
    assert math.isnan(mean_pair_distance(torch.zeros(1, 1))) and math.isnan(mean_pair_distance(torch.zeros(0, 0)))
    d = torch.tensor([[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [2.0, 3.0, 0.0]])
    assert mean_pair_distance(d) == 2.0
    assert nan_mean([math.nan, 2.0, 4.0, math.nan]) == 3.0
    assert math.isnan(nan_mean([math.nan, math.nan]))


class _StubG(torch.nn.Module):
    """g_ema stand-in: image i of a call = a fixed function of its latent."""

    def __init__(self, size):
        super().__init__()
        self.size = size
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.calls = 0

    def forward(self, zs):
        z = zs[0]
        self.calls += 1
        n = z.shape[0]
        base = torch.tanh(z[:, :3]).view(n, 3, 1, 1)
        ramp = torch.linspace(-0.2, 0.2, self.size).view(1, 1, 1, -1)
        return (base * 0.8 + ramp).expand(n, 3, self.size, self.size).contiguous(), None


class _StubLpips:
    """Features = the scaled images; distance = mean squared difference (a stand-in for the VGG network)."""
    workspace_features = None
    batch = 1

    class F:
        def __init__(self, x):
            self.x = x

    def features(self, x, quantize=False, out=None, u8_out=None):
        from rick_amd.lpips import scale_input
        xs, q = scale_input(x, quantize)
        if u8_out is not None:
            u8_out.copy_(q)
        return self.F(xs)

    def distances(self, a, b):
        return ((a.x[:, None] - b.x[None]) ** 2).flatten(2).mean(2)


def test_intra_lpips_cluster_procedure_with_stubbed_distances():
    from rick_amd.evaluate import intra_lpips
    size, K = 16, 4
    g = _StubG(size)
    latents = torch.randn(70, 8, generator=torch.Generator().manual_seed(3))
    centers = (torch.rand(K, 3, size, size, generator=torch.Generator().manual_seed(4)) * 255).to(torch.uint8)
    stub = _StubLpips()
    val, per, counts = intra_lpips(g, centers, stub, n_samples=60, n_sample_store=7, cluster_size=8, size=size, latents=latents,
                                   rng=torch.Generator().manual_seed(5))
    assert g.calls == 9 and int(counts.sum()) == 63                # 9 batches of 7 >= 60
    # restatement: quantise, nearest centre, subset, mean over unordered pairs
    imgs = torch.cat([g([latents[i:i + 7]])[0] for i in range(0, 63, 7)])
    q = ((imgs / 2 + 0.5) * 255 + 0.5).clamp(0, 255).to(torch.uint8)
    xs = [stub.features(q).x, stub.features(centers).x]
    d = stub.distances(stub.F(xs[0]), stub.F(xs[1])).double()
    assign = torch.from_numpy(np.argmin(d.numpy(), 1))
    assert torch.equal(counts, torch.bincount(assign, minlength=K))
    rng = torch.Generator().manual_seed(5)
    ref = []
    for c in range(K):
        m = torch.nonzero(assign == c).flatten()
        if m.numel() > 8:
            m = m[torch.randperm(m.numel(), generator=rng)[:8]]
        if m.numel() < 2:
            ref.append(math.nan)
            continue
        dd = stub.distances(stub.F(xs[0][m]), stub.F(xs[0][m])).double()
        ref.append(float(dd[torch.triu(torch.ones(len(m), len(m), dtype=torch.bool), 1)].mean()))
    ref = torch.tensor(ref, dtype=torch.float64)
    assert torch.equal(torch.isnan(per), torch.isnan(ref))
    ok = ~torch.isnan(ref)
    assert torch.allclose(per[ok], ref[ok], rtol=1e-12, atol=0)
    assert abs(val - float(ref[ok].mean())) <= 1e-12 * abs(val)
    with pytest.raises(ValueError):
        intra_lpips(g, centers[:, :, :8, :8], stub, n_samples=7, n_sample_store=7, size=size, latents=latents)
    with pytest.raises(ValueError):
        intra_lpips(g, torch.zeros(K, 3, 32, 32, dtype=torch.uint8), stub, n_samples=7, n_sample_store=7, size=32,
                    latents=latents)


def test_intra_lpips_on_the_cpu_network():
    """The real (CPU) network end to end at 16 px: a cluster value equals the fp64 pair mean of its members."""
    from rick_amd.evaluate import intra_lpips
    from rick_amd.lpips import LPIPS
    sd = synthetic_state_dict(2)
    net = LPIPS.load(sd, device='cpu')
    g = _StubG(16)
    latents = torch.randn(12, 8, generator=torch.Generator().manual_seed(9))
    centers = ((smooth_images(2, 16, seed=11) / 2 + 0.5) * 255).to(torch.uint8)
    val, per, counts = intra_lpips(g, centers, net, n_samples=12, n_sample_store=6, cluster_size=50, size=16, latents=latents)
    assert int(counts.sum()) == 12
    imgs = g([latents])[0]
    q = ((imgs / 2 + 0.5) * 255 + 0.5).clamp(0, 255).to(torch.uint8)
    dc = lpips_matrix_f64(sd, (q.double() / 255 - 0.5) / 0.5, (centers.double() / 255 - 0.5) / 0.5)
    assign = dc.argmin(1)
    assert torch.equal(counts, torch.bincount(assign, minlength=2))
    for c in range(2):
        m = torch.nonzero(assign == c).flatten()
        if m.numel() < 2:
            assert math.isnan(per[c])
            continue
        x = (q[m].double() / 255 - 0.5) / 0.5
        dd = lpips_matrix_f64(sd, x, x)
        ref = float(dd[torch.triu(torch.ones(len(m), len(m), dtype=torch.bool), 1)].mean())
        assert abs(float(per[c]) - ref) <= 1e-5 * abs(ref)


def test_load_cluster_centers(tmp_path):
    from rick_amd.data import encode_png
    from rick_amd.evaluate import load_cluster_centers
    g = np.random.RandomState(0)
    imgs = g.randint(0, 256, (3, 12, 12, 3)).astype(np.uint8)
    for i, im in enumerate(imgs):
        os.makedirs(tmp_path / f'c{i}')
        (tmp_path / f'c{i}' / 'center.png').write_bytes(encode_png(im, filter_type=i % 5))
        (tmp_path / f'c{i}' / '000001.png').write_bytes(encode_png(im[::-1].copy()))      # assigned samples are ignored
    got = load_cluster_centers(str(tmp_path), k=3)
    assert got.dtype == torch.uint8 and got.shape == (3, 3, 12, 12)
    assert np.array_equal(got.permute(0, 2, 3, 1).numpy(), imgs)
    with pytest.raises(FileNotFoundError):
        load_cluster_centers(str(tmp_path), k=4)
