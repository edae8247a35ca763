"""CPU: the perceptual path length (rick_amd/ppl.py) — the fp64 restatement's own sanity (tests/ppl_f64.py), the percentile filter
against NumPy, PathLengthStats' independence of the batching, the CPU path of the whole metric against the restatement, every
validation error, and the two new C symbols.

The generator of the metric tests is the architecture of ``Generator(32, 512, 2, channel_multiplier=1)`` with synthetic weights.
The HIP generator has no CPU path, so here the same weights run through the oracle's functional generator behind the module's
interface (tests/ppl_f64.RefGenerator); tests/test_gpu_ppl.py runs the module itself."""
import os
import re

import numpy as np
import pytest
import torch

from rick_amd.synth import synth_state_dict
from tests import ppl_f64
from tests.lpips_f64 import synthetic_state_dict
from tests.shapes import generator_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 32


def _ab(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, L, generator=g), torch.randn(B, L, generator=g)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_sanity():
    a, b = _ab(4, 64, 0)
    b[1] = a[1]
    t = torch.tensor([0.0, 0.3, 0.5, 1.0])
    out = ppl_f64.path_latents(a, b, t, 1e-4, 'z')
    assert out.dtype == torch.float64 and out.shape == (8, 64) and torch.isfinite(out).all()
    assert float((out.norm(dim=1) - 1).abs().max()) <= 1e-14                       # unit rows
    an, bn = ppl_f64.normalize(a.double()), ppl_f64.normalize(b.double())
    assert float((out[0] - an[0]).abs().max()) <= 1e-15                            # t = 0 gives a / |a|
    assert float((out[2] - an[1]).abs().max()) <= 1e-7                             # a == b stays at an: finite, no NaN
    assert float((out[6] - bn[3]).abs().max()) <= 1e-14                            # t = 1 gives b / |b|
    # the two rows of a pair are eps apart along the arc: |out[2i + 1] - out[2i]| = 2 sin(eps theta / 2)
    theta = torch.acos((an * bn).sum(1).clamp(-1, 1))
    step = (out[1::2] - out[0::2]).norm(dim=1)
    assert float((step - 2 * torch.sin(1e-4 * theta / 2)).abs().max()) <= 1e-12
    w = ppl_f64.path_latents(a, b, torch.tensor([0.0, 1.0, 0.5, 0.25]), 0.5, 'w')
    assert torch.equal(w[0], a[0].double()) and float((w[2] - b[1].double()).abs().max()) <= 1e-15   # lerp end points
    assert float((w[5] - b[2].double()).abs().max()) <= 1e-15                      # t + eps = 1


@pytest.mark.parametrize('n', [3, 100, 101, 257])
def test_percentile_filter_matches_numpy(n):
    from rick_amd.ppl import PathLengthStats, percentile_indices
    g = torch.Generator().manual_seed(n)
    for ties in (False, True):
        d = torch.rand(n, generator=g) * 100
        if ties:
            d = (d / 10).round() * 10          # 11 distinct values: the percentiles fall inside runs of equal values
        x = d.double().numpy()
        lo, hi = np.percentile(x, 1, method='lower'), np.percentile(x, 99, method='higher')
        want = x[(x >= lo) & (x <= hi)]
        want = float(np.sum(np.sort(want).astype(np.longdouble)) / len(want))
        assert ppl_f64.filtered_mean(d.tolist()) == pytest.approx(want, rel=1e-15)
        s = np.sort(x)
        i_lo, i_hi = percentile_indices(n)
        assert s[i_lo] == lo and s[i_hi] == hi
        got, kept = PathLengthStats(n, 'cpu').update(d).finalize()
        assert got == ppl_f64.filtered_mean(d.tolist()) and torch.equal(kept, d)
    if n > 100:                                # the filter does remove something there
        assert ppl_f64.filtered_mean(range(n)) == (n - 1) / 2 and percentile_indices(n) != (0, n - 1)


def test_percentile_indices_match_numpy_for_every_small_n():
    from rick_amd.ppl import percentile_indices
    for n in list(range(2, 1200)) + [5000, 10000, 50000]:
        x = np.arange(n, dtype=np.float64)
        assert percentile_indices(n) == (int(np.percentile(x, 1, method='lower')), int(np.percentile(x, 99, method='higher'))), n


def test_stats_do_not_depend_on_the_batching():
    from rick_amd.ppl import PathLengthStats
    d = torch.rand(257, generator=torch.Generator().manual_seed(1)) ** 4 * 1e3
    one = PathLengthStats(257, 'cpu').update(d).finalize()
    st = PathLengthStats(257, 'cpu')
    for lo in range(0, 257, 25):
        st.update(d[lo:lo + 25])
    many = st.finalize()
    assert one[0] == many[0] and torch.equal(one[1], many[1])
    perm = torch.randperm(257, generator=torch.Generator().manual_seed(2))
    assert PathLengthStats(257, 'cpu').update(d[perm]).finalize()[0] == one[0]
    with pytest.raises(RuntimeError, match='ppl.PathLengthStats'):
        PathLengthStats(5, 'cpu').update(d[:3]).finalize()
    with pytest.raises(ValueError, match='ppl.PathLengthStats'):
        PathLengthStats(5, 'cpu').update(d[:6])


# ---- the CPU path of the metric -------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def world():
    from rick_amd.lpips import LPIPS
    sg = synth_state_dict(generator_shapes(SIZE, n_mlp=2, cm=1))
    sl = synthetic_state_dict(3)
    return sg, sl, ppl_f64.RefGenerator(sg, SIZE), LPIPS.load(sl, device='cpu', batch=8, size=SIZE)


@pytest.mark.parametrize('crop', [False, True])
@pytest.mark.parametrize('sampling', ['end', 'full'])
@pytest.mark.parametrize('space', ['w', 'z'])
def test_cpu_metric_vs_fp64(world, space, sampling, crop):
    """6 paths at batch 4 (a short last batch), eps = 1e-2.  Bound: 4 x the deviation of the plain fp32 composition
    (tests/ppl_f64.py evaluated in float32) from its float64 evaluation, per path relative to the fp64 value, on these paths."""
    from rick_amd.ppl import perceptual_path_length
    sg, sl, g, net = world
    n, eps = 6, 1e-2
    latents, noise = ppl_f64.pinned_paths(n, SIZE, 11, sampling)
    ref = ppl_f64.path_distances(sg, sl, SIZE, *latents, noise, eps, space, crop)
    f32 = ppl_f64.path_distances(sg, sl, SIZE, *latents, noise, eps, space, crop, dtype=torch.float32)
    assert ref.dtype == torch.float64 and f32.dtype == torch.float32 and bool((ref > 0).all())
    g.train()
    ppl, d = perceptual_path_length(g, net, n_samples=n, batch=4, eps=eps, space=space, sampling=sampling, crop=crop,
                                    latents=latents, noise=noise)
    assert g.training                                                   # the generator's mode is restored
    assert d.shape == (n,) and d.dtype == torch.float32
    yard = float(((f32.double() - ref).abs() / ref).max())
    err = float(((d.double() - ref).abs() / ref).max())
    print(f'ppl cpu {space}/{sampling}/crop={crop}: rel err {err:.2e}, fp32 composition {yard:.2e}, values {ref.min():.3g} .. {ref.max():.3g}')
    assert yard > 0 and err <= 4 * yard
    want = ppl_f64.filtered_mean(ref.tolist())
    assert abs(ppl - want) <= 4 * yard * want
    assert ppl == ppl_f64.filtered_mean(d.tolist())


def test_cpu_path_latents_and_paired(world):
    from rick_amd.ppl import draw_paths, path_latents
    _, _, _, net = world
    a, b = _ab(5, 512, 3)
    t = torch.tensor([0.0, 0.5, 0.99, 0.25, 1.0])
    for space in ('w', 'z'):
        got = path_latents(a, b, t, 1e-2, space)
        ref = ppl_f64.path_latents(a, b, t, 1e-2, space)
        assert got.dtype == torch.float32 and float((got.double() - ref).abs().max()) <= 1e-6
    z0, z1, tt = draw_paths(7, 512, 'full', torch.Generator().manual_seed(0))
    assert z0.shape == z1.shape == (7, 512) and tt.shape == (7,) and bool(((tt >= 0) & (tt < 1)).all()) and not torch.equal(z0, z1)
    assert torch.equal(draw_paths(7, 512, 'end')[2], torch.zeros(7))
    x = torch.rand(4, 3, 16, 16, generator=torch.Generator().manual_seed(4)) * 2 - 1
    f = net.features(x)
    inter = net.paired(f)
    assert inter.shape == (2,) and torch.allclose(inter, torch.diagonal(net.distances(f.narrow(0, 4), f.narrow(0, 4))[0::2, 1::2]),
                                                  rtol=1e-5)
    assert torch.allclose(net.paired(net.features(x[0::2]), net.features(x[1::2])), inter, rtol=1e-5)
    assert torch.allclose(net(x[0::2], x[1::2]), inter, rtol=1e-5)


# ---- validation -----------------------------------------------------------------------------------------------------------
def test_validation_errors(world):
    from rick_amd.ppl import PathLengthStats, draw_paths, path_latents, perceptual_path_length
    _, _, g, net = world
    a, b = _ab(3, 8, 0)
    t = torch.zeros(3)
    for bad in (dict(space='x'), dict(eps=0.0), dict(eps=-1e-4), dict(eps=float('inf')), dict(eps=float('nan')),
                dict(a=a[:, :4]), dict(a=a[0]), dict(t=t[:2]), dict(t=t[:, None]), dict(a=a.double()), dict(t=t.double())):
        kw = dict(a=a, b=b, t=t, eps=1e-4, space='w')
        kw.update(bad)
        with pytest.raises(ValueError, match=r'ppl\.path_latents'):
            path_latents(**kw)
    with pytest.raises(ValueError, match=r'ppl\.draw_paths'):
        draw_paths(4, 512, 'middle')
    with pytest.raises(ValueError, match=r'ppl\.draw_paths'):
        draw_paths(0, 512, 'end')
    with pytest.raises(ValueError, match=r'ppl\.PathLengthStats.*too few'):
        PathLengthStats(1, 'cpu')
    latents, noise = ppl_f64.pinned_paths(4, SIZE, 0)
    ok = dict(n_samples=4, batch=2, eps=1e-2, latents=latents, noise=noise)
    for bad, msg in ((dict(space='x'), 'space'), (dict(sampling='x'), 'sampling'), (dict(eps=0), 'eps'),
                     (dict(n_samples=1), 'too small'), (dict(batch=0), 'batch'), (dict(n_samples=5), 'latents'),
                     (dict(latents=(latents[0][:, :8], latents[1][:, :8], latents[2])), 'latents'),
                     (dict(noise=noise[:-1]), 'noise'), (dict(noise=[m[:3] for m in noise]), 'noise')):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError, match=r'ppl\.perceptual_path_length.*' + msg):
            perceptual_path_length(g, net, **kw)
    x = torch.rand(3, 3, 16, 16) * 2 - 1
    with pytest.raises(RuntimeError, match=r'LPIPS\.paired.*3 images'):
        net.paired(net.features(x))
    with pytest.raises(RuntimeError, match=r'LPIPS\.paired'):
        net.paired(net.features(x), net.features(x[:2]))


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported():
    from rick_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'rick_hip.h')).read()
    for name in ('rick_ppl_latents_f32', 'rick_lpips_paired_f32'):
        assert re.search(r'^int ' + name + r'\(', text, re.M), f'{name} is not declared in rick_hip.h'
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
