"""CPU: the VGG16 fc2 loader and weight layouts, the nearest-resize index rule against F.interpolate, the CPU network
against the independent fp64 restatement (tests/vgg_f64.py), and the evaluator's precision / recall through
``pr_feature_fn``."""
import pytest
import torch
import torch.nn.functional as F

from tests.vgg_f64 import SmoothG, fc2_f64, max_rel_err, pr_margin, smooth_images, synthetic_vgg16_state_dict

SIZES = [256, 224, 299, 64, 200]
# fp32 torch composition against fp64, max error over max-norm.  A sequential fp32 sum of K zero-mean terms has an rms relative
# error of u sqrt(K / 6), u = 2^-24; over the network's 15 layers (K = 27, 2 x 576, 2 x 1152, 3 x 2304, 5 x 4608, 25088, 4096)
# these add in quadrature to u sqrt(10436) = 102 u = 6.1e-6 if every sum were one sequential chain (blocked BLAS sums are
# shorter).  The bound leaves a factor 3 for a maximum over 8192 features against that rms estimate.  A wrong layer, order,
# permutation or resize is an O(1) error.
CPU_BOUND = 2e-5


@pytest.fixture(scope='module')
def sd():
    return synthetic_vgg16_state_dict(0)


@pytest.fixture(scope='module')
def net(sd):
    from rick_amd.vgg import VGG16Fc2Features
    return VGG16Fc2Features.load(sd, device='cpu', batch=4)


def test_restatement_is_alive(sd):
    """A dead network (all-zero or constant features) would pass every comparison below."""
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)) * 2 - 1
    f = fc2_f64(sd, x)
    assert tuple(f.shape) == (2, 4096) and torch.isfinite(f).all()
    assert 0.1 < float(f.std()) < 10, float(f.std())
    assert float((f[0] - f[1]).abs().max()) > 1e-3 * float(f.abs().max())
    assert float(f[0].max() - f[0].min()) > 0.1


def test_loader_takes_the_torchvision_layout(sd, tmp_path):
    from rick_amd.vgg import VGG16Fc2Features
    a = VGG16Fc2Features.load(sd, device='cpu')
    assert sorted(a.convs) == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    for idx in a.convs:
        assert torch.equal(a.convs[idx][0], sd[f'features.{idx}.weight']) and torch.equal(a.convs[idx][1], sd[f'features.{idx}.bias'])
    for (w, b), idx in zip(a.fcs, (0, 3)):
        assert torch.equal(w, sd[f'classifier.{idx}.weight']) and torch.equal(b, sd[f'classifier.{idx}.bias'])
    # classifier.6 is accepted and ignored
    full = dict(sd, **{'classifier.6.weight': torch.ones(1000, 4096), 'classifier.6.bias': torch.ones(1000)})
    b = VGG16Fc2Features.load(full, device='cpu')
    x = smooth_images(1, 32, seed=3)
    assert torch.equal(a(x), b(x))
    # from a file
    small = tmp_path / 'vgg16.pth'
    torch.save(sd, small)
    c = VGG16Fc2Features.load(str(small), device='cpu')
    assert torch.equal(c.fcs[1][0], a.fcs[1][0])


def test_loader_names_wrong_shapes_missing_and_unknown_keys(sd):
    from rick_amd.vgg import VGG16Fc2Features
    with pytest.raises(RuntimeError, match='classifier.0.weight'):
        VGG16Fc2Features.load(dict(sd, **{'classifier.0.weight': torch.zeros(4096, 4096)}), device='cpu')
    with pytest.raises(RuntimeError, match='features.10.weight'):
        VGG16Fc2Features.load(dict(sd, **{'features.10.weight': torch.zeros(256, 128, 1, 1)}), device='cpu')
    with pytest.raises(RuntimeError, match='classifier.3.bias'):
        VGG16Fc2Features.load({k: v for k, v in sd.items() if k != 'classifier.3.bias'}, device='cpu')
    with pytest.raises(RuntimeError, match='features.28.weight'):
        VGG16Fc2Features.load({k: v for k, v in sd.items() if k != 'features.28.weight'}, device='cpu')
    with pytest.raises(RuntimeError, match='features.30.weight'):
        VGG16Fc2Features.load(dict(sd, **{'features.30.weight': torch.zeros(1)}), device='cpu')
    with pytest.raises(RuntimeError, match='classifier.7.weight'):
        VGG16Fc2Features.load(dict(sd, **{'classifier.7.weight': torch.zeros(1)}), device='cpu')


def test_fc1_permutation_matches_the_nhwc_flatten():
    """permute_fc1 moves fc1's K axis from the reference's (c, y, x) flatten to the trunk's NHWC (y, x, c) one."""
    from rick_amd.vgg import FC_IN, permute_fc1
    w = torch.arange(3 * FC_IN, dtype=torch.float32).view(3, FC_IN)
    p = permute_fc1(w)
    f = torch.randint(-4, 5, (2, 512, 7, 7), generator=torch.Generator().manual_seed(0)).double()     # integers: sums are exact
    ref = f.reshape(2, FC_IN) @ w.double().t()                               # the reference's .view(-1, 7 * 7 * 512)
    got = f.permute(0, 2, 3, 1).reshape(2, FC_IN) @ p.double().t()           # the trunk's [n, 7, 7, 512]
    assert torch.equal(got, ref)
    c, y, x = 37, 5, 2
    assert torch.equal(p[:, (y * 7 + x) * 512 + c], w[:, c * 49 + y * 7 + x])


@pytest.mark.parametrize('n,k', [(4096, 4096), (200, 1000), (64, 512), (5, 13)])
def test_packed_fc_weight_layout(n, k):
    """Lane (h, c) of column block nb and k block kb holds W[32 nb + c][8 kb + 2 j + h] in component j; zero padding."""
    from rick_amd.vgg import pack_fc_weight
    w = torch.arange(1, n * k + 1, dtype=torch.float32).view(n, k)
    np_, kp = -(-n // 128) * 128, -(-k // 8) * 8
    pk = pack_fc_weight(w).view(np_ // 32, kp // 8, 2, 32, 4)
    g = torch.Generator().manual_seed(n)
    for _ in range(200):
        nb, kb, h, c, j = (int(torch.randint(0, hi, (1,), generator=g)) for hi in (np_ // 32, kp // 8, 2, 32, 4))
        row, col = 32 * nb + c, 8 * kb + 2 * j + h
        want = float(w[row, col]) if row < n and col < k else 0.0
        assert float(pk[nb, kb, h, c, j]) == want
    assert float(pk.sum(dtype=torch.float64)) == float(w.sum(dtype=torch.float64))


@pytest.mark.parametrize('hw', [(s, s) for s in SIZES] + [(100, 317)])
def test_nearest_indices_equal_interpolate(hw):
    from rick_amd.vgg import nearest_index, resize_nearest
    h, w = hw
    x = torch.arange(2 * 3 * h * w, dtype=torch.float32).view(2, 3, h, w)
    ref = F.interpolate(x, size=(224, 224))
    assert torch.equal(resize_nearest(x), ref)
    iy, ix = nearest_index(h), nearest_index(w)
    assert iy.dtype == torch.int64 and tuple(iy.shape) == (224,) and int(iy.max()) <= h - 1 and int(ix.max()) <= w - 1
    assert torch.equal(x[:, :, iy][:, :, :, ix], ref)
    if h == 224:
        assert torch.equal(iy, torch.arange(224))


@pytest.mark.parametrize('size', [64, 256])
def test_cpu_path_vs_fp64(sd, net, size):
    x = smooth_images(2, size, seed=size)
    ref = fc2_f64(sd, x)
    got = net(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 4096)
    err = max_rel_err(got, ref)
    print(f'cpu fc2 features at {size}^2: max err / max-norm {err:.2e}')
    assert err <= CPU_BOUND


def test_any_n_is_chunked_at_batch(sd, net):
    x = smooth_images(6, 32, seed=9)              # batch = 4: two chunks
    got = net(x)
    assert tuple(got.shape) == (6, 4096)
    assert max_rel_err(got, fc2_f64(sd, x)) <= CPU_BOUND
    assert tuple(net(x[:0]).shape) == (0, 4096)
    with pytest.raises(RuntimeError):
        net(x[:, :2])
    with pytest.raises(RuntimeError):
        net(x.double())


def test_evaluator_precision_recall_through_pr_feature_fn(sd, net):
    """Evaluator(pr_feature_fn=net, real_pr_feats=net(real)) == precision_recall_from_features on the fp64 restatement's
    features, and differs from what the Inception fallback (feature_fn's features) gives on the same samples."""
    from rick_amd.evaluate import Evaluator, precision_recall_from_features
    n_real, n_fake, size, k = 14, 12, 32, 3
    g = SmoothG(size)
    z = torch.randn(n_fake, 512, generator=torch.Generator().manual_seed(39))
    real = smooth_images(n_real, size, seed=40, low=4) * 0.9
    with torch.no_grad():
        fake = g([z])[0]
    fr64, ff64 = fc2_f64(sd, real), fc2_f64(sd, fake)
    # the condition under which fp32 features cannot flip a count: a condition on the sample set, not a tolerance
    margin = pr_margin(fr64, ff64, k)
    print(f'precision / recall margin of the sample set: {margin:.2e}')
    assert margin > 1e-4
    p_ref, r_ref = (float(v) for v in precision_recall_from_features(fr64, ff64, k=k))

    proj = torch.randn(3 * 16, 8, generator=torch.Generator().manual_seed(23), dtype=torch.float64)

    def feature_fn(img):                          # stands in for Inception pool3
        return F.adaptive_avg_pool2d(img.double(), 4).flatten(1) @ proj
    kw = dict(n_sample_store=6, inception_nsamples=n_fake, fid_sample_size=n_fake, k=k)
    ev = Evaluator(g, feature_fn, feature_fn(real), pr_feature_fn=net, real_pr_feats=net(real), **kw)
    got = ev.compute_inception_score(fid=False, pr=True, latents=z)
    assert (float(got['precision']), float(got['recall'])) == (p_ref, r_ref)
    fallback = Evaluator(g, feature_fn, feature_fn(real), **kw).compute_inception_score(fid=False, pr=True, latents=z)
    assert (float(fallback['precision']), float(fallback['recall'])) != (p_ref, r_ref)
    assert 0 < p_ref + r_ref < 2                  # not the trivial all-in / all-out answer on both sides
