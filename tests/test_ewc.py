"""rick_amd.ewc on the CPU: the anchor's layout and checks, its in-place state_dict round trip, the torch composition of the
penalty against the NumPy fp64 restatement tests/ewc_f64.py, and the trainer's configuration checks.  CPU-only; the kernels and
the whole G step with the term run in tests/test_gpu_ewc.py.

Tolerances are those of tests/ewc_f64.py: 3 * 2^-24 (|g0| + |term|) per gradient element (the CPU composition rounds once, the
kernel three times), n * 2^-52 * value for the sum."""
import numpy as np
import pytest
import torch

from tests import ewc_f64

# registration order; sizes that are no multiple of the 64-float alignment, one of them larger than it, one a single element
SHAPES = [('head.w', (5,)), ('convs.0.w', (3, 5)), ('convs.0.b', (1,)), ('convs.1.w', (2, 3, 11)), ('convs.1.b', (65,)),
          ('tail.w', (7,))]
OPT = [n for n, _ in SHAPES if 'convs' in n]


def _flat(seed=0):
    from rick_amd.train import FlatParams
    g = torch.Generator().manual_seed(seed)
    named = [(n, torch.nn.Parameter(torch.randn(*s, generator=g))) for n, s in SHAPES]
    return FlatParams(named, lambda n: 'convs' in n)


def _maps(flat, seed=1, delta=1e-2):
    g = torch.Generator().manual_seed(seed)
    src = {n: p.detach() + delta * torch.randn(p.shape, generator=g) for n, p in zip(flat.names, flat.params)}
    fis = {n: 1e-2 * torch.rand(p.shape, generator=g) for n, p in zip(flat.names, flat.params)}
    return src, fis


def test_anchor_has_the_layout_of_the_optimised_slice():
    from rick_amd.ewc import EwcAnchor
    flat = _flat()
    src, fis = _maps(flat)
    a = EwcAnchor(flat, src, fis)
    assert a.names == OPT and (a.lo, a.hi) == (flat.lo, flat.hi) and a.n == flat.hi - flat.lo
    assert a.anchor.shape == a.fisher.shape == (a.n,) and a.anchor.dtype == a.fisher.dtype == torch.float32
    covered = torch.zeros(a.n, dtype=torch.bool)
    for name in OPT:
        i = flat.index[name]
        lo, hi = a.segment(name)
        assert lo == int(flat.offsets[i]) - flat.lo and hi - lo == flat.sizes[i]
        assert torch.equal(a.anchor[lo:hi], src[name].reshape(-1)) and torch.equal(a.fisher[lo:hi], fis[name].reshape(-1))
        covered[lo:hi] = True
    assert (~covered).any()                                    # there IS padding at these sizes
    assert not a.anchor[~covered].any() and not a.fisher[~covered].any()
    assert a.value.dtype == torch.float64 and a.value.dim() == 0 and a.partials.dtype == torch.float64
    # fisher=None: ones on the parameters (L2-SP), still zero in the padding
    ones = EwcAnchor(flat, src)
    assert torch.equal(ones.fisher, covered.to(torch.float32))


def test_anchor_error_paths():
    from rick_amd.ewc import EwcAnchor
    flat = _flat()
    src, fis = _maps(flat)
    EwcAnchor(flat, {n: src[n] for n in OPT}, {n: fis[n] for n in OPT})          # entries of other parameters are not needed
    with pytest.raises(KeyError, match='convs.1.w'):
        EwcAnchor(flat, {n: v for n, v in src.items() if n != 'convs.1.w'}, fis)
    with pytest.raises(KeyError, match='convs.0.b'):
        EwcAnchor(flat, src, {n: v for n, v in fis.items() if n != 'convs.0.b'})
    with pytest.raises(ValueError, match='convs.0.w'):
        EwcAnchor(flat, dict(src, **{'convs.0.w': torch.zeros(5, 3)}), fis)      # same size, wrong shape
    with pytest.raises(ValueError, match='convs.1.b'):
        EwcAnchor(flat, src, dict(fis, **{'convs.1.b': torch.zeros(64)}))
    for bad in (-1e-9, float('nan'), float('inf')):
        f = fis['convs.1.w'].clone()
        f[1, 2, 3] = bad
        with pytest.raises(ValueError, match='convs.1.w'):
            EwcAnchor(flat, src, dict(fis, **{'convs.1.w': f}))
    with pytest.raises(ValueError, match='convs.0.b'):
        EwcAnchor(flat, dict(src, **{'convs.0.b': torch.empty(1, device='meta')}), fis)
    with pytest.raises(ValueError, match='convs.0.w'):
        EwcAnchor(flat, src, dict(fis, **{'convs.0.w': torch.empty(3, 5, device='meta')}))


def test_state_dict_round_trip_is_in_place():
    from rick_amd.ewc import EwcAnchor
    flat = _flat()
    src, fis = _maps(flat)
    a = EwcAnchor(flat, src, fis)
    sd = a.state_dict()
    assert sorted(sd) == sorted([f'anchor.{n}' for n in OPT] + [f'fisher.{n}' for n in OPT])
    assert all(sd[f'anchor.{n}'].shape == src[n].shape and torch.equal(sd[f'fisher.{n}'], fis[n]) for n in OPT)
    b = EwcAnchor(flat, *_maps(flat, seed=5))
    assert not torch.equal(a.anchor, b.anchor) and not torch.equal(a.fisher, b.fisher)
    ptrs = (b.anchor.data_ptr(), b.fisher.data_ptr(), b.partials.data_ptr(), b.value.data_ptr())
    b.load_state_dict(sd)
    assert torch.equal(a.anchor, b.anchor) and torch.equal(a.fisher, b.fisher)
    assert ptrs == (b.anchor.data_ptr(), b.fisher.data_ptr(), b.partials.data_ptr(), b.value.data_ptr())
    sd['anchor.convs.0.w'].zero_()                             # state_dict() hands out copies
    assert a.anchor[slice(*a.segment('convs.0.w'))].any()
    # a state that fails a check changes nothing
    bad = dict(a.state_dict())
    bad['fisher.convs.1.b'] = -bad['fisher.convs.1.b'] - 1.0
    bad['anchor.convs.0.w'] = bad['anchor.convs.0.w'] + 1.0
    with pytest.raises(ValueError, match='convs.1.b'):
        b.load_state_dict(bad)
    del bad['fisher.convs.1.b']
    with pytest.raises(KeyError, match='convs.1.b'):
        b.load_state_dict(bad)
    assert torch.equal(a.anchor, b.anchor) and torch.equal(a.fisher, b.fisher)


@pytest.mark.parametrize('masked', [False, True], ids=['no_mask', 'mask'])
@pytest.mark.parametrize('weight', [1.0, 5e8 * 1e-8, 0.0])
def test_cpu_penalty_equals_the_fp64_restatement(weight, masked):
    from rick_amd.ewc import EwcAnchor, penalty_
    flat = _flat()
    src, fis = _maps(flat)
    fis['convs.1.w'][0] = 0.0                                  # Fisher zeros among the entries
    a = EwcAnchor(flat, src, fis)
    g = torch.Generator().manual_seed(3)
    flat.grad.copy_(torch.randn(flat.total, generator=g))
    mask = torch.randint(0, 4, (a.n,), generator=g).to(torch.uint8) if masked else None
    theta = flat.flat[a.lo:a.hi].numpy().copy()
    g0 = flat.grad.numpy().copy()
    v = penalty_(a, weight, mask)
    assert v is a.value and v.dtype == torch.float64
    m = None if mask is None else mask.numpy()
    vref = ewc_f64.value(theta, a.anchor.numpy(), a.fisher.numpy(), m)
    term = ewc_f64.grad_term(theta, a.anchor.numpy(), a.fisher.numpy(), weight, m)
    assert vref > 0 and abs(float(v) - vref) <= ewc_f64.value_bound(a.n, vref)
    got = flat.grad.numpy().astype(np.float64)
    s = slice(a.lo, a.hi)
    assert (np.abs(got[s] - (g0[s].astype(np.float64) + term)) <= ewc_f64.grad_bound(g0[s], term)).all()
    if weight:
        assert np.abs(term).max() > 1e2 * ewc_f64.grad_bound(g0[s], term).max()        # the bound would notice a missing term
    keep = ewc_f64.kept(m, a.n)
    assert np.array_equal(got[s][~keep], g0[s][~keep]) and (weight == 0 or (got[s][keep & (term != 0)] != g0[s][keep & (term != 0)]).any())
    assert np.array_equal(got[:a.lo], g0[:a.lo]) and np.array_equal(got[a.hi:], g0[a.hi:])    # nothing outside the slice
    assert np.array_equal(flat.flat[a.lo:a.hi].numpy(), theta)
    if weight == 0:
        assert np.array_equal(got, g0)


def test_penalty_argument_checks():
    from rick_amd.ewc import EwcAnchor, accumulate_, penalty_
    flat = _flat()
    a = EwcAnchor(flat, *_maps(flat))
    for w in (-1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            penalty_(a, w)
    with pytest.raises(ValueError):
        penalty_(a, 1.0, torch.zeros(a.n - 1, dtype=torch.uint8))
    with pytest.raises(ValueError):
        penalty_(a, 1.0, torch.zeros(a.n, dtype=torch.int32))
    x = torch.zeros(8)
    with pytest.raises(ValueError):
        accumulate_(x, x, x[:7], x.clone(), 1.0)
    with pytest.raises(ValueError):
        accumulate_(x, x, x.double(), x.clone(), 1.0)
    assert float(accumulate_(x[:0], x[:0], x[:0], x[:0].clone(), 1.0)) == 0.0


def test_blocks_is_a_function_of_n_alone():
    from rick_amd._lib import lib
    ns = [0, 1, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 5, 1 << 20, (1 << 31) + 1, 1 << 40]
    b = [lib.rick_ewc_blocks(n) for n in ns]
    assert b[0] == 0 and b[1] == 1 and b == sorted(b) and all(k * 4096 >= n > (k - 1) * 4096 for k, n in zip(b[1:], ns[1:]))
    assert lib.rick_ewc_blocks(-1) < 0


def test_c_entries_refuse_null_pointers_and_negative_sizes():
    """RICK_EINVAL (22) before anything is launched: no GPU involved."""
    from rick_amd._lib import lib
    ok = 4096                                                  # any aligned non-null address: the checks come first
    assert lib.rick_ewc_f32(None, ok, ok, ok, None, 4, 1.0, ok, None) == 22
    assert lib.rick_ewc_f32(ok, None, ok, ok, None, 4, 1.0, ok, None) == 22
    assert lib.rick_ewc_f32(ok, ok, None, ok, None, 4, 1.0, ok, None) == 22
    assert lib.rick_ewc_f32(ok, ok, ok, None, None, 4, 1.0, ok, None) == 22
    assert lib.rick_ewc_f32(ok, ok, ok, ok, None, 4, 1.0, None, None) == 22
    assert lib.rick_ewc_f32(ok, ok, ok, ok, None, -1, 1.0, ok, None) == 22
    assert lib.rick_ewc_f32(ok + 2, ok, ok, ok, None, 4, 1.0, ok, None) == 22
    assert lib.rick_ewc_f32(ok, ok, ok, ok, None, 0, 1.0, ok, None) == 0       # n == 0 launches nothing
    assert lib.rick_ewc_finish_f64(None, 1, ok, None) == 22
    assert lib.rick_ewc_finish_f64(ok, 1, None, None) == 22
    assert lib.rick_ewc_finish_f64(ok, -1, ok, None) == 22


# ---- trainer -------------------------------------------------------------------------------------------------------------------
def _nets(size=32):
    from rick_amd.models import Discriminator, Generator
    torch.manual_seed(0)
    g0 = Generator(size, 512, 2, channel_multiplier=1)

    def build():
        g, d = Generator(size, 512, 2, channel_multiplier=1), Discriminator(size, channel_multiplier=1)
        g.load_state_dict(g0.state_dict())
        return g, d
    return build, {k: v.clone() for k, v in g0.state_dict().items()}


def _trainer(weight, ewc):
    from rick_amd.train import RickTrainer, TrainConfig
    build, _ = _nets()
    g, d = build()
    g_ema, d_ema = build()
    return RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, ewc_weight=weight), g, d, g_ema, d_ema, ewc=ewc)


def test_ewc_weight_validation():
    from rick_amd.ewc import EwcAnchor
    from rick_amd.train import TrainConfig, g_optim_filter
    assert TrainConfig().ewc_weight == 0.0
    _, state = _nets()
    for w in (-1.0, float('nan')):
        with pytest.raises(ValueError, match='ewc_weight'):
            _trainer(w, (state, None))
    with pytest.raises(ValueError, match='ewc'):
        _trainer(5.0, None)
    off = _trainer(0.0, None)
    assert off.ewc is None and off.g_optim.before_step is None
    tr = _trainer(5.0, (state, None))
    assert isinstance(tr.ewc, EwcAnchor) and tr.ewc.flat is tr.g_flat
    assert tr.ewc.names == [n for n, _ in tr.g.named_parameters() if g_optim_filter(n)]
    lo, hi = tr.ewc.segment('convs.0.conv.weight')
    assert torch.equal(tr.ewc.anchor[lo:hi], state['convs.0.conv.weight'].reshape(-1)) and bool((tr.ewc.fisher[lo:hi] == 1).all())
    # the anchor can be replaced after construction: by mappings, or by an anchor built on the trainer's own flat buffer
    fis = {n: torch.full_like(p, 0.5) for n, p in tr.g.named_parameters()}
    second = tr.set_ewc(state, fis)
    assert tr.ewc is second and bool((second.fisher[lo:hi] == 0.5).all())
    third = EwcAnchor(tr.g_flat, state)
    assert tr.set_ewc(third) is third and tr.ewc is third
    with pytest.raises(ValueError, match='g_flat'):
        tr.set_ewc(EwcAnchor(off.g_flat, state))
    with pytest.raises(KeyError):
        tr.set_ewc({k: v for k, v in state.items() if k != 'convs.0.conv.weight'})
    assert tr.ewc is third
    # the capture signature carries the switch and the weight
    assert tr._graph_signature(tr.g_optim) != off._graph_signature(off.g_optim)


def test_before_step_runs_at_the_top_of_the_optimiser_step():
    """MaskedFlatAdam.before_step on an optimiser that owns no parameter (its step launches nothing, so it runs on the CPU)."""
    from rick_amd.train import FlatParams, MaskedFlatAdam
    flat = FlatParams([('a', torch.nn.Parameter(torch.zeros(3)))], lambda n: False)
    opt = MaskedFlatAdam(flat, 1e-3, (0.0, 0.99))
    calls = []
    opt.step()
    opt.before_step = lambda: calls.append(list(opt.last_runs))
    opt.last_runs = ['stale']
    opt.step()
    assert calls == [['stale']] and opt.last_runs == []        # called once, before the step did anything
