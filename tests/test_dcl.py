"""rick_amd/dcl.py without a device: the fp64 composition path of xgram and both contrastive losses against the literal
restatement tests/dcl_f64.py, the invariances of the losses, the C ABI's argument checks on the cross-built library, and the
trainer's validation and forward-pair sharing with stand-in generators (tests/test_feature_pair.py's)."""
import ctypes

import numpy as np
import pytest
import torch

from rick_amd import cdc, dcl
from tests.dcl_f64 import cl1_f64, cl2_f64, random_feats

SHAPES = [(8, 4, 4), (16, 8, 8), (5, 7, 9), (3, 33, 31)]
# The composition path accumulates in fp64 on fp32 inputs, the restatement is fp64 throughout: what separates them is fp64
# rounding in sums of up to 3 * 33 * 31 terms and a softmax at 1 / tau = 14: 1e-11 is far above that and far below fp32.
TOL = 1e-11
EINVAL = 22


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max())


def test_xgram_composition_vs_fp64_and_layouts():
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(3, 6, 5, 7, generator=g) + 1, torch.randn(5, 6, 5, 7, generator=g) + 1
    A, B = a.flatten(1).double(), b.flatten(1).double()
    for x, y in ((a, b), (a.contiguous(memory_format=torch.channels_last), b.contiguous(memory_format=torch.channels_last)),
                 (a.contiguous(memory_format=torch.channels_last), b)):          # the last pair: b is brought into a's layout
        x, y = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
        C, na, nb = dcl.xgram(x, y)
        assert C.dtype == na.dtype == nb.dtype == torch.float64 and C.shape == (3, 5) and na.shape == (3,) and nb.shape == (5,)
        assert _rel(C, A @ B.t()) <= TOL and _rel(na, (A * A).sum(1)) <= TOL and _rel(nb, (B * B).sum(1)) <= TOL
        w, u, v = torch.randn(3, 5, generator=g).double(), torch.randn(3, generator=g).double(), torch.randn(5, generator=g).double()
        gx, gy = torch.autograd.grad((C * w).sum() + (na * u).sum() + (nb * v).sum(), (x, y))
        assert gx.shape == x.shape and gx.stride() == x.stride()                 # the gradient in the layout of its operand
        assert _rel(gx, (w @ B + 2 * u[:, None] * A).view_as(a)) <= 2.0 ** -23 + TOL
        assert _rel(gy, (w.t() @ A + 2 * v[:, None] * B).view_as(b)) <= 2.0 ** -23 + TOL


def test_xgram_reads_two_halves_of_one_tensor_in_place():
    f = torch.randn(8, 3, 4, 4, generator=torch.Generator().manual_seed(1)).contiguous(memory_format=torch.channels_last)
    a, b = f[:4], f[4:]
    assert cdc._sample_dense(a) and cdc._sample_dense(b) and dcl._same_layout(a, b)
    assert cdc._rows(b).data_ptr() == b.data_ptr() and cdc._rows(a).data_ptr() == f.data_ptr()
    C, na, nb = dcl.xgram(a, b)
    G = cdc.gram(f)
    assert _rel(C, G[:4, 4:]) <= TOL and _rel(na, torch.diagonal(G)[:4]) <= TOL and _rel(nb, torch.diagonal(G)[4:]) <= TOL


def _cl1_case(layers, B=4, seed=3):
    fs = random_feats(SHAPES, B, seed)
    ft = [f + 0.3 * torch.randn(f.shape, generator=torch.Generator().manual_seed(seed + k)) for k, f in enumerate(fs)]
    return ft, fs, layers


def _cl2_case(layers, B=4, M=4, seed=5):
    gen = torch.Generator().manual_seed(seed)
    pos = random_feats(SHAPES, B, seed)
    anc = [f + 0.3 * torch.randn(f.shape, generator=gen) for f in pos]
    neg = [torch.randn(M, *s, generator=gen) * 0.5 + f[:1] for f, s in zip(pos, SHAPES)]
    return anc, pos, neg, layers


@pytest.mark.parametrize('layers', [[0, 1, 2, 3], [2, 0, 2, 2]], ids=['distinct', 'repeated'])
def test_cl1_value_and_gradient_vs_restatement(layers):
    ft, fs, _ = _cl1_case(layers)
    used = sorted(set(layers))
    t64 = [f.double().requires_grad_(True) for f in ft]
    ref = cl1_f64(t64, fs, layers)
    gref = torch.autograd.grad(ref, [t64[l] for l in used])
    t32 = [f.clone().requires_grad_(True) for f in ft]
    s32 = [f.clone().requires_grad_(True) for f in fs]
    loss = dcl.generator_contrastive_loss(t32, s32, layers, 0.07)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and float(ref) > 0
    assert abs(float(loss) - float(ref)) <= 2.0 ** -23 * abs(float(ref)) + TOL
    loss.backward()
    assert all(f.grad is None for f in s32)                                      # gradients flow into the target features only
    for l, r in zip(used, gref):
        assert _rel(t32[l].grad, r) <= 2.0 ** -22


@pytest.mark.parametrize('layers', [[0, 1, 2, 3], [3, 1, 3, 3]], ids=['distinct', 'repeated'])
def test_cl2_value_and_gradients_vs_restatement(layers):
    anc, pos, neg, _ = _cl2_case(layers)
    used = sorted(set(layers))
    a64, n64 = [f.double().requires_grad_(True) for f in anc], [f.double().requires_grad_(True) for f in neg]
    ref = cl2_f64(a64, pos, n64, layers)
    gref = torch.autograd.grad(ref, [a64[l] for l in used] + [n64[l] for l in used])
    a32, n32 = [f.clone().requires_grad_(True) for f in anc], [f.clone().requires_grad_(True) for f in neg]
    p32 = [f.clone().requires_grad_(True) for f in pos]
    loss = dcl.discriminator_contrastive_loss(a32, p32, n32, layers, 0.07)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and float(ref) > 0
    assert abs(float(loss) - float(ref)) <= 2.0 ** -23 * abs(float(ref)) + TOL
    loss.backward()
    assert all(f.grad is None for f in p32)                                      # the positives take no gradient
    for t, r in zip([a32[l] for l in used] + [n32[l] for l in used], gref):
        assert _rel(t.grad, r) <= 2.0 ** -22


def test_cl1_of_one_sample_is_exactly_zero():
    ft, fs, _ = _cl1_case([2], B=1)
    ft = [f.requires_grad_(True) for f in ft]
    loss = dcl.generator_contrastive_loss(ft, fs, [2])
    assert float(loss) == 0.0
    (g,) = torch.autograd.grad(loss, ft[2])
    assert not g.any()


def test_losses_do_not_change_with_a_samples_scale():
    layers = [2, 0, 2, 1]
    ft, fs, _ = _cl1_case(layers)
    base = dcl.generator_contrastive_loss(ft, fs, layers).double()
    ft2, fs2 = [f.clone() for f in ft], [f.clone() for f in fs]
    for l in range(len(SHAPES)):
        ft2[l][1] *= 3.0                                                         # powers of two and others: cos is scale-free
        fs2[l][2] *= 0.37
    assert abs(float(dcl.generator_contrastive_loss(ft2, fs2, layers)) - float(base)) <= 4 * 2.0 ** -23 * float(base)
    anc, pos, neg, _ = _cl2_case(layers)
    base = dcl.discriminator_contrastive_loss(anc, pos, neg, layers)
    a2, p2, n2 = [f.clone() for f in anc], [f.clone() for f in pos], [f.clone() for f in neg]
    for l in range(len(SHAPES)):
        a2[l][0] *= 5.0
        p2[l][3] *= 0.11
        n2[l][2] *= 7.0
    assert abs(float(dcl.discriminator_contrastive_loss(a2, p2, n2, layers)) - float(base)) <= 4 * 2.0 ** -23 * float(base)


def test_cl2_does_not_depend_on_the_order_of_the_negatives():
    layers = [3, 1, 3, 0]
    anc, pos, neg, _ = _cl2_case(layers)
    base = dcl.discriminator_contrastive_loss(anc, pos, neg, layers)
    perm = [2, 0, 3, 1]
    got = dcl.discriminator_contrastive_loss(anc, pos, [f[perm].contiguous() for f in neg], layers)
    assert abs(float(got) - float(base)) <= 2 * 2.0 ** -23 * float(base)         # the softmax adds the same terms in another order


def test_create_graph_raises():
    a = torch.randn(3, 10, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    b = torch.randn(2, 10, generator=torch.Generator().manual_seed(2))
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(dcl.xgram(a, b)[0].sum(), a, create_graph=True)


def test_refusals():
    with pytest.raises(RuntimeError):
        dcl.xgram(torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3))
    with pytest.raises(RuntimeError):
        dcl.xgram(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.float16))
    with pytest.raises(ValueError):
        dcl.xgram(torch.zeros(0, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError):
        dcl.xgram(torch.zeros(2, 3), torch.zeros(2, 4))
    with pytest.raises(ValueError):
        dcl.generator_contrastive_loss([torch.zeros(3, 5)], [torch.zeros(3, 5)], [0, 0])
    with pytest.raises(ValueError):
        dcl.generator_contrastive_loss([torch.zeros(2, 5)], [torch.zeros(2, 5)], [0, 0], tau=0.0)
    with pytest.raises(ValueError):
        dcl.discriminator_contrastive_loss([torch.zeros(2, 5)], [torch.zeros(3, 5)], [torch.zeros(4, 5)], [0, 0])


def test_draw_d_layers_is_uniform_over_the_whole_list():
    np.random.seed(4)
    got = dcl.draw_d_layers(14, 6)
    assert np.array_equal(got, np.random.RandomState(4).randint(0, 14, size=6))
    rng = np.random.RandomState(9)
    seen = set(int(l) for l in dcl.draw_d_layers(14, 4000, rng))
    assert seen == set(range(14))
    assert np.array_equal(dcl.draw_d_layers(14, 5, np.random.RandomState(1)), np.random.RandomState(1).randint(0, 14, size=5))


# ---- C ABI on the cross-built library: every refusal comes before any launch, no device involved ------------------------------
def test_c_abi_symbols_and_argument_checks():
    from rick_amd import _lib
    lib = _lib.lib
    for name in ('rick_xgram_workspace_bytes', 'rick_xgram_f32', 'rick_xrowmix_f32'):
        assert hasattr(lib, name)
    assert lib.rick_xgram_workspace_bytes(0, 4, 100) == -1
    assert lib.rick_xgram_workspace_bytes(4, 9, 100) == -1
    assert lib.rick_xgram_workspace_bytes(4, 4, 0) == -1
    assert lib.rick_xgram_workspace_bytes(4, 4, 4097) == 2 * (16 + 8) * 4                      # two slices of 24 products
    assert lib.rick_xgram_workspace_bytes(8, 8, 4096 * 1024 + 1) == 513 * 80 * 4               # the slices have grown to 8192
    buf = (ctypes.c_double * 4096)()
    p = ctypes.addressof(buf)
    a, b, ws, C, na, nb, y = p, p + 1024, p + 2048, p + 4096, p + 5120, p + 6144, p + 8192
    ok = (a, 2, b, 2, 16, ws, C, na, nb, None)
    for k in (0, 2, 5, 6, 7, 8):                                                               # each pointer null in turn
        args = list(ok)
        args[k] = None
        assert lib.rick_xgram_f32(*args) == EINVAL
    assert lib.rick_xgram_f32(a + 2, 2, b, 2, 16, ws, C, na, nb, None) == EINVAL               # a at 2 bytes
    assert lib.rick_xgram_f32(a, 2, b, 2, 16, ws, C + 4, na, nb, None) == EINVAL               # an fp64 output at 4 bytes
    assert lib.rick_xgram_f32(a, 0, b, 2, 16, ws, C, na, nb, None) == EINVAL
    assert lib.rick_xgram_f32(a, 2, b, 9, 16, ws, C, na, nb, None) == EINVAL
    assert lib.rick_xgram_f32(a, 2, b, 2, 0, ws, C, na, nb, None) == EINVAL
    M, d = ws, ws + 512
    ok = (M, d, a, b, y, 2, 2, 16, None)
    for k in range(5):
        args = list(ok)
        args[k] = None
        assert lib.rick_xrowmix_f32(*args) == EINVAL
    assert lib.rick_xrowmix_f32(M, d, a, b, a, 2, 2, 16, None) == EINVAL                       # y == a
    assert lib.rick_xrowmix_f32(M, d, a, b, b, 2, 2, 16, None) == EINVAL                       # y == b
    assert lib.rick_xrowmix_f32(M, d, a, b, a + 64, 2, 2, 16, None) == EINVAL                  # y inside a's second row
    assert lib.rick_xrowmix_f32(M, d, a, b, y + 2, 2, 2, 16, None) == EINVAL                   # misaligned
    assert lib.rick_xrowmix_f32(M, d, a, b, y, 9, 2, 16, None) == EINVAL
    assert lib.rick_xrowmix_f32(M, d, a, b, y, 2, 0, 16, None) == EINVAL
    assert lib.rick_xrowmix_f32(M, d, a, b, y, 2, 2, 0, None) == EINVAL


# ---- trainer --------------------------------------------------------------------------------------------------------------------
def _build(size=32):
    from rick_amd.models import Discriminator, Generator
    torch.manual_seed(0)
    g0 = Generator(size, 512, 2, channel_multiplier=1)

    def build():
        g, d = Generator(size, 512, 2, channel_multiplier=1), Discriminator(size, channel_multiplier=1)
        g.load_state_dict(g0.state_dict())
        return g, d
    return build


def _make(g_source=True, d_source=True, **cfg):
    from rick_amd.train import RickTrainer, TrainConfig
    build = _build()
    g, d = build()
    g_ema, d_ema = build()
    gs, ds = build()
    gs, ds = (gs if g_source else None), (ds if d_source else None)
    tr = RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, **cfg), g, d, g_ema, d_ema, g_source=gs, d_source=ds)
    return tr, gs, ds


def test_config_defaults_are_off():
    from rick_amd.train import TrainConfig
    c = TrainConfig()
    assert c.dcl_g_weight == 0.0 and c.dcl_d_weight == 0.0 and c.dcl_tau == 0.07 and c.dcl_batch == 4


def test_trainer_validation():
    from rick_amd.train import RickTrainer
    with pytest.raises(ValueError, match='g_source'):
        _make(g_source=False, dcl_g_weight=2.0)
    with pytest.raises(ValueError, match='d_source'):
        _make(d_source=False, dcl_d_weight=0.5)
    with pytest.raises(ValueError, match='g_source'):
        _make(g_source=False, dcl_d_weight=0.5)
    with pytest.raises(ValueError, match='augment or diffaug'):
        _make(dcl_d_weight=0.5, augment=True)
    with pytest.raises(ValueError, match='augment or diffaug'):
        _make(dcl_d_weight=0.5, diffaug='color')
    _make(dcl_g_weight=2.0, augment=True)                                        # the generator term goes with augmentation
    for bad in (dict(dcl_g_weight=-1.0), dict(dcl_d_weight=-0.5), dict(dcl_g_weight=float('nan')), dict(dcl_g_weight=1.0, dcl_tau=0.0),
                dict(dcl_tau=-0.07), dict(dcl_batch=0)):
        with pytest.raises(ValueError, match='dcl_'):
            _make(**bad)
    tr, gs, ds = _make(dcl_g_weight=2.0, dcl_d_weight=0.5)
    for src in (gs, ds):                                                         # both frozen alike
        assert not src.training and not any(p.requires_grad for p in src.parameters())
    with pytest.raises(ValueError, match='d_source'):
        RickTrainer(tr.cfg, tr.g, tr.d, tr.g_ema, tr.d_ema, g_source=gs, d_source=tr.d)
    _make(g_source=False, d_source=False)                                        # everything off: no source network needed


def _stand_in(gen, calls):
    ws = [p for n, p in gen.named_parameters() if n.startswith('convs.') and n.endswith('conv.weight')]

    def forward(styles, return_feats=False, noise=None, **kw):
        calls.append((torch.is_grad_enabled(), noise, styles[0]))
        z = styles[0]
        feats = [torch.tanh(z[:, k:k + 48].reshape(-1, 3, 4, 4) + (k + 1.0) * ws[k % len(ws)].flatten()[:48].view(1, 3, 4, 4)) + 1.0
                 for k in range(gen.n_latent - 1)]
        return None, feats
    return forward


def _stood_in(**cfg):
    tr, gs, _ = _make(**cfg)
    with torch.no_grad():
        for p in tr.g.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
    t_calls, s_calls = [], []
    tr.g.forward, gs.forward = _stand_in(tr.g, t_calls), _stand_in(gs, s_calls)
    return tr, gs, t_calls, s_calls


def _terms(tr, g_noise=None, **draws):
    """The unweighted values of the trainer's G-step terms (rick_amd/gterms.py), evaluated the way g_step's loop does."""
    memo, out = {}, {}
    for term in tr.g_terms:
        out.update({name: value for name, (_, value) in term(draws, g_noise, memo).items()})
    assert not memo                                                              # what was handed on was taken
    return out


def test_cl1_term_uses_one_forward_pair_and_the_source_without_grad():
    tr, gs, t_calls, s_calls = _stood_in(dcl_g_weight=2.0, dcl_batch=4)
    z = torch.randn(4, 512, generator=torch.Generator().manual_seed(2))
    layers, maps = [1, 3, 3, 5], object()
    term = _terms(tr, maps, dcl_noise=z, dcl_layers=layers)['dcl_g']
    assert len(t_calls) == 1 and len(s_calls) == 1
    assert t_calls[0][:2] == (True, maps) and s_calls[0][:2] == (False, maps) and t_calls[0][2] is z and s_calls[0][2] is z
    feats_t, feats_s = tr._feature_pair(z)
    assert torch.equal(term.detach(), dcl.generator_contrastive_loss(feats_t, feats_s, layers, tr.cfg.dcl_tau).detach())
    assert float(term) > 0
    term.backward()
    got = [n for n, p in tr.g.named_parameters() if p.grad is not None and p.grad.any()]
    assert got and all(n.startswith('convs.') for n in got)
    assert all(p.grad is None for p in gs.parameters())
    # the draws when none are given: dcl_batch latents, layers from cdc.draw_layers
    del t_calls[:], s_calls[:]
    np.random.seed(0)
    term = _terms(tr)['dcl_g']
    z = t_calls[0][2]
    assert z.shape == (4, 512) and s_calls[0][2] is z
    feats_t, feats_s = tr._feature_pair(z)
    want = dcl.generator_contrastive_loss(feats_t, feats_s, np.random.RandomState(0).randint(1, tr.g.n_latent - 1, 4), tr.cfg.dcl_tau)
    assert torch.equal(term.detach(), want.detach())


def test_cdc_and_cl1_share_the_pair_when_their_batches_agree():
    tr, gs, t_calls, s_calls = _stood_in(dcl_g_weight=2.0, dcl_batch=4, cdc_weight=1000.0, cdc_batch=4)
    z = torch.randn(4, 512, generator=torch.Generator().manual_seed(2))
    terms = _terms(tr, cdc_noise=z, cdc_layers=[1, 3, 3, 5], dcl_layers=[2, 2, 4, 1])
    assert len(t_calls) == 1 and len(s_calls) == 1 and s_calls[0][0] is False
    feats_t, feats_s = tr._feature_pair(z)
    assert torch.equal(terms['cdc'].detach(), cdc.distance_consistency_loss(feats_t, feats_s, [1, 3, 3, 5]).detach())
    assert torch.equal(terms['dcl_g'].detach(), dcl.generator_contrastive_loss(feats_t, feats_s, [2, 2, 4, 1], 0.07).detach())
    del t_calls[:], s_calls[:]
    terms = _terms(tr)                                              # nothing given: one drawn z for both
    assert len(t_calls) == 1 and len(s_calls) == 1 and set(terms) == {'cdc', 'dcl_g'}
    # batches that differ: each term makes its own pair
    tr, gs, t_calls, s_calls = _stood_in(dcl_g_weight=2.0, dcl_batch=3, cdc_weight=1000.0, cdc_batch=4)
    terms = _terms(tr)
    assert sorted(c[2].shape[0] for c in t_calls) == [3, 4] and len(s_calls) == 2 and set(terms) == {'cdc', 'dcl_g'}
    # one term on: only its own
    tr, gs, t_calls, s_calls = _stood_in(dcl_g_weight=2.0, dcl_batch=4)
    assert set(_terms(tr)) == {'dcl_g'} and len(t_calls) == 1


@pytest.mark.parametrize('dcl_batch', [3, 4])
def test_both_terms_consume_their_draws_in_the_fixed_order(dcl_batch):
    """No draws given, both terms on: the torch stream gives the distance-consistency term's latents first and then, when the
    batches differ (no shared pair), CL1's; numpy's global stream gives the distance-consistency term's layers first, then
    CL1's.  (The stand-ins draw no noise maps.)  Both values equal the losses on the draws replayed by hand in that order."""
    seed = 5
    tr, gs, t_calls, s_calls = _stood_in(dcl_g_weight=2.0, dcl_batch=dcl_batch, cdc_weight=1000.0, cdc_batch=4)
    torch.manual_seed(seed)
    np.random.seed(seed)
    terms = _terms(tr)
    shared = dcl_batch == 4
    assert len(t_calls) == len(s_calls) == (1 if shared else 2)
    torch.manual_seed(seed)
    z_cdc = torch.randn(4, 512)
    z_dcl = z_cdc if shared else torch.randn(dcl_batch, 512)
    got_cdc, got_dcl = t_calls[0][2], t_calls[-1][2]                             # read back before the replay records more calls
    assert torch.equal(got_cdc, z_cdc) and torch.equal(got_dcl, z_dcl)
    assert all(t[2] is s[2] for t, s in zip(t_calls, s_calls))
    rng = np.random.RandomState(seed)
    layers_cdc = rng.randint(1, tr.g.n_latent - 1, 4)
    layers_dcl = rng.randint(1, tr.g.n_latent - 1, dcl_batch)
    with torch.no_grad():
        want_cdc = cdc.distance_consistency_loss(*tr._feature_pair(got_cdc), layers_cdc)
        want_dcl = dcl.generator_contrastive_loss(*tr._feature_pair(got_dcl), layers_dcl, tr.cfg.dcl_tau)
    assert torch.equal(terms['cdc'].detach(), want_cdc) and torch.equal(terms['dcl_g'].detach(), want_dcl)
    assert float(want_cdc) > 0 and float(want_dcl) > 0


def test_g_step_refuses_a_keyword_no_term_declares():
    from rick_amd import gterms
    assert gterms.DRAWS == {'cdc_noise', 'cdc_layers', 'dcl_noise', 'dcl_layers', 'clip_noise'}
    tr, gs, t_calls, s_calls = _stood_in(dcl_g_weight=2.0)
    with pytest.raises(TypeError, match='bogus'):
        tr.g_step(None, bogus=1)                                                 # before any work: these networks have no CPU path
    with pytest.raises(TypeError, match='bogus'):
        tr.g_step(None, cdc_noise=None, bogus=1)                                 # next to a declared keyword of a term that is off
    assert not t_calls and not s_calls
