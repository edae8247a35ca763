"""CPU: the Inception Score path (rick_amd.inception.InceptionV3Logits, rick_amd.evaluate.InceptionScoreStats) — loader, the
fp32 torch composition against the fp64 restatement (tests/inception_score_f64.py), the statistic's bookkeeping and the
Evaluator's 'is' / 'is_std'.

Tolerances.  The base figure of a comparison is the error of the fp32 torch CPU composition against the fp64 restatement on
the same inputs, measured once and written down in CPU_BASE: for the logits max |d| over the fp64 max-norm, for the score the
relative error.  A score is a single number, so its error is a single draw that can come out near zero by accident, and the
mean and the std over two splits are (s1 + s2) / 2 and |s1 - s2| / 2, in which the splits' errors can cancel or add up.  The
score base of a case is therefore the largest relative error among the scores the checks are made of: the whole set's
(splits 1) and each half's (splits 2).  It bounds the mean's error relative to the mean and the std's error relative to the
larger split score, mean + std.  The bound is the base x 4, which covers another blocking of the same fp32 sums (another
BLAS, another thread count)."""
import pytest
import torch

from tests.inception_f64 import synthetic_state_dict, wrapper_layout
from tests.inception_score_f64 import score_f64, score_from_preds, smooth_images, softmax_f64_of_f32, with_head

# case -> ((n, h, w, seed) of smooth_images, size argument of load); shared with tests/test_gpu_inception_score.py
CASES = {'native80x96': ((4, 80, 96, 11), (80, 96)), 'resize64': ((4, 64, 64, 12), None), 'native75': ((4, 75, 75, 13), (75, 75)),
         'native75n70': ((70, 75, 75, 14), (75, 75))}
# fp32 torch CPU composition against fp64: (logits max |d| / max-norm, score relative error: the largest of the whole set's
# and the two halves')
CPU_BASE = {'native80x96': (4.737e-06, 3.263e-07), 'resize64': (7.701e-06, 8.338e-07), 'native75': (4.844e-06, 2.121e-07),
            'native75n70': (5.677e-06, 4.564e-07)}
FACTOR = 4


def case(name):
    """-> (images, size, state_dict with the fitted head, fp64 logits)."""
    spec, size = CASES[name]
    images = smooth_images(*spec)
    sd, ref = with_head(images, size, key=name)
    return images, size, sd, ref


def max_rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


# ---- loader ---------------------------------------------------------------------------------------------------------------
def _with_fc(sd):
    sd = dict(sd)
    g = torch.Generator().manual_seed(3)
    sd['fc.weight'], sd['fc.bias'] = torch.randn(1000, 2048, generator=g) * 0.05, torch.randn(1000, generator=g)
    return sd


def test_loader_accepts_both_layouts():
    from rick_amd.inception import InceptionV3Logits
    sd = _with_fc(synthetic_state_dict(0))
    a = InceptionV3Logits.load(sd, device='cpu', size=(75, 75))
    wrapped = wrapper_layout(sd)
    assert not any(k.startswith('fc.') for k in wrapped)
    wrapped.update({'fc.weight': sd['fc.weight'], 'fc.bias': sd['fc.bias']})
    b = InceptionV3Logits.load(wrapped, device='cpu', size=(75, 75))
    assert torch.equal(a.fc[0], b.fc[0]) and torch.equal(a.fc[1], b.fc[1])
    assert all(torch.equal(a.folded[k][0], b.folded[k][0]) and torch.equal(a.folded[k][1], b.folded[k][1]) for k in a.folded)
    x = smooth_images(2, 75, 75, 5)
    assert torch.equal(a(x), b(x)) and tuple(a(x).shape) == (2, 1000)


def test_loader_names_a_missing_or_misshaped_fc_key():
    from rick_amd.inception import InceptionV3Logits
    sd = _with_fc(synthetic_state_dict(0))
    bad = dict(sd)
    del bad['fc.bias']
    with pytest.raises(KeyError, match='fc.bias'):
        InceptionV3Logits.load(bad, device='cpu')
    bad = dict(sd)
    bad['fc.weight'] = sd['fc.weight'][:, :2047]
    with pytest.raises(ValueError, match='fc.weight'):
        InceptionV3Logits.load(bad, device='cpu')
    bad = dict(sd)
    del bad['Mixed_7c.branch_pool.conv.weight']
    with pytest.raises(KeyError, match='Mixed_7c.branch_pool.conv.weight'):
        InceptionV3Logits.load(bad, device='cpu')


def test_size_is_checked():
    from rick_amd.inception import InceptionV3Logits
    sd = _with_fc(synthetic_state_dict(0))
    with pytest.raises(ValueError):
        InceptionV3Logits.load(sd, device='cpu', size=(74, 80))
    net = InceptionV3Logits.load(sd, device='cpu', size=(80, 96))
    with pytest.raises(RuntimeError, match='80, 96'):
        net(torch.zeros(1, 3, 96, 80))
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 80, 96, dtype=torch.float64))


def test_pack_fc_weight_has_one_home():
    from rick_amd import fc, vgg
    assert vgg.pack_fc_weight is fc.pack_fc_weight and vgg.FC_MAX_ROWS == fc.FC_MAX_ROWS == 64


# ---- the fp32 composition against fp64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['native80x96', 'resize64'])
def test_cpu_logits_and_score_vs_fp64(name):
    from rick_amd.evaluate import inception_score
    from rick_amd.inception import InceptionV3Logits
    images, size, sd, ref = case(name)
    net = InceptionV3Logits.load(sd, device='cpu', batch=3, size=size)            # chunks of 3 + 1
    got = net(images)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 1000)
    base, sbase = CPU_BASE[name]
    err = max_rel(got, ref)
    print(f'{name}: CPU logits max err / max-norm {err:.3e} (base {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.allclose(net.probs(images), torch.softmax(got, -1), rtol=0, atol=0)
    for splits in (1, 2):
        want = score_f64(ref, splits)
        assert want[0] > 1.5
        mean, std = inception_score(images, net, splits)
        assert mean.dtype == torch.float64 and std.dtype == torch.float64
        rel = abs(float(mean) - want[0]) / want[0]
        print(f'{name}: CPU score splits {splits}: {float(mean):.6f} (fp64 {want[0]:.6f}) rel {rel:.3e} '
              f'(base {sbase:.3e}, bound {FACTOR * sbase:.3e})')
        assert rel <= FACTOR * sbase
        assert abs(float(std) - want[1]) <= FACTOR * sbase * (want[0] + want[1])
        # the streamed state evaluates the reference's own expression on the same fp32 softmax
        restated = score_from_preds(softmax_f64_of_f32(got), splits)
        assert abs(float(mean) - restated[0]) <= 1e-12 * restated[0] and abs(float(std) - restated[1]) <= 1e-12 * restated[0]


# ---- bookkeeping of the statistic -------------------------------------------------------------------------------------------
def _logits(n, c, seed=0):
    return torch.randn(n, c, generator=torch.Generator().manual_seed(seed)) * 3


def _stats(logits, n_total, splits, cuts):
    from rick_amd.evaluate import InceptionScoreStats
    st = InceptionScoreStats(lambda z: z, n_total, splits)            # the 'network' hands the rows through
    lo = 0
    for m in cuts:
        st.update(logits[lo:lo + m])
        lo += m
    return st


def test_splits_drop_the_remainder_and_std_is_the_population_std():
    z = _logits(10, 37)
    st = _stats(z, 10, 3, [10])
    assert st.per == 3 and tuple(st.acc.shape) == (3, 75)
    mean, std = st.finalize()
    want = score_from_preds(softmax_f64_of_f32(z), 3)
    assert abs(float(mean) - want[0]) <= 1e-12 * want[0] and abs(float(std) - want[1]) <= 1e-12 * want[0]
    assert want[1] > 0
    # row 9 is dropped: another last row, the same state
    z2 = z.clone()
    z2[9] = -z[9]
    assert torch.equal(_stats(z2, 10, 3, [10]).acc, st.acc)
    # every split is the score of its own three rows; np.std is the population std
    per_split = [score_from_preds(softmax_f64_of_f32(z[3 * k:3 * k + 3]), 1)[0] for k in range(3)]
    t = torch.tensor(per_split, dtype=torch.float64)
    assert abs(float(mean) - float(t.mean())) <= 1e-12 * want[0]
    assert abs(float(std) - float(t.std(unbiased=False))) <= 1e-12 * want[0]
    one = _stats(z, 10, 1, [10]).finalize()
    assert float(one[1]) == 0.0


def test_state_does_not_depend_on_the_cut():
    z = _logits(10, 37, seed=1)
    whole = _stats(z, 10, 3, [10])
    assert torch.equal(_stats(z, 10, 3, [4, 6]).acc, whole.acc)
    assert torch.equal(_stats(z, 10, 3, [1] * 10).acc, whole.acc)
    a, b = _stats(z, 10, 3, [4, 6]).finalize(), whole.finalize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_underflowing_softmax_stays_finite():
    z = _logits(6, 37, seed=2)
    z[2, 5] = z[2].max() + 200                                        # p underflows to exactly 0 elsewhere in this row
    assert int((torch.softmax(z, -1)[2] == 0).sum()) == 36
    st = _stats(z, 6, 2, [6])
    mean, std = st.finalize()
    assert bool(torch.isfinite(st.acc).all()) and bool(torch.isfinite(mean)) and bool(torch.isfinite(std))
    want = score_from_preds(softmax_f64_of_f32(z), 2)
    assert abs(float(mean) - want[0]) <= 1e-12 * want[0] and abs(float(std) - want[1]) <= 1e-12 * want[0]
    # every row certain of the same class: zeros in the marginal too, score exactly 1
    z = torch.zeros(4, 9)
    z[:, 3] = 300
    mean, _ = _stats(z, 4, 1, [4]).finalize()
    assert float(mean) == 1.0


def test_arguments_are_checked():
    from rick_amd.evaluate import InceptionScoreStats
    with pytest.raises(ValueError):
        InceptionScoreStats(lambda z: z, 10, 0)
    with pytest.raises(ValueError):
        InceptionScoreStats(lambda z: z, 2, 3)
    st = _stats(_logits(4, 5), 10, 3, [4])
    with pytest.raises(RuntimeError, match='4 of 9'):
        st.finalize()


# ---- Evaluator --------------------------------------------------------------------------------------------------------------
class _G(torch.nn.Module):
    """A stand-in generator: latents -> images [n, 3, 75, 75] in [-1, 1]."""
    size = 75

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.randn(512, 3 * 5 * 5, generator=torch.Generator().manual_seed(9)) * 0.1)

    def forward(self, styles):
        x = torch.tanh(styles[0] @ self.w).view(-1, 3, 5, 5)
        return torch.nn.functional.interpolate(x, size=(75, 75), mode='bilinear', align_corners=False), None


def test_evaluator_reports_the_score_of_the_first_sample_size_images():
    from rick_amd.evaluate import Evaluator, InceptionScoreStats
    from rick_amd.inception import InceptionV3Logits
    net = InceptionV3Logits.load(_with_fc(synthetic_state_dict(0)), device='cpu', size=(75, 75))
    g = _G()
    z = torch.randn(9, 512, generator=torch.Generator().manual_seed(4))
    feature_fn = lambda img: img.mean((2, 3))                                   # noqa: E731
    real = torch.randn(8, 3, generator=torch.Generator().manual_seed(5))
    ev = Evaluator(g, feature_fn, real, n_sample_store=3, inception_nsamples=9, fid_sample_size=7, is_net=net)
    got = ev.compute_inception_score(fid=True, latents=z, iscore=True, is_splits=2)
    assert set(got) == {'fid', 'is', 'is_std'}
    st = InceptionScoreStats(net, 7, 2)
    with torch.no_grad():
        for lo, take in ((0, 3), (3, 3), (6, 1)):                               # the first 7 of the 9 generated images
            st.update(g([z[lo:lo + 3]])[0][:take])
    mean, std = st.finalize()
    assert torch.equal(got['is'], mean) and torch.equal(got['is_std'], std)
    assert float(mean) > 1.0
    # the defaults are today's behaviour: the same keys, the same FID, no is_net needed
    plain = Evaluator(g, feature_fn, real, n_sample_store=3, inception_nsamples=9, fid_sample_size=7)
    off = plain.compute_inception_score(fid=True, latents=z)
    assert set(off) == {'fid'} and torch.equal(off['fid'], got['fid'])
    assert set(ev.compute_inception_score(fid=True, latents=z)) == {'fid'}
    with pytest.raises(RuntimeError, match='is_net'):
        plain.compute_inception_score(fid=False, latents=z, iscore=True)
