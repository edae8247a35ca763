"""rick_amd.kml on the CPU: the torch fp64 composition of apply_ / grads_ against the NumPy restatement tests/kml_f64.py and
against torch autograd through W0 * (1 + a @ b.T)[..., None], the set_rows rules, the in-place state_dict round trip and every
validation error.  CPU-only; the kernels and the trainer run in tests/test_gpu_kml.py.

Tolerances are those of tests/kml_f64.py (the CPU composition rounds once per element, far inside them); every test prints the
measured error as a fraction of its bound (run with -s)."""
import numpy as np
import pytest
import torch

from tests import kml_f64

# registration order: a bias in between, a 5-D generator weight, a 1x1 skip, a 2-D weight that is only modulated when named
SHAPES = [('head.w', (4, 3, 3, 3)), ('convs.0.w', (6, 5, 3, 3)), ('convs.0.b', (6,)), ('convs.1.w', (1, 7, 4, 3, 3)),
          ('convs.2.skip', (9, 8, 1, 1)), ('convs.3.fc', (5, 11)), ('tail.w', (7,))]
DEFAULT = ['convs.0.w', 'convs.1.w', 'convs.2.skip']
R = 2


def _flat(seed=0):
    from rick_amd.train import FlatParams
    g = torch.Generator().manual_seed(seed)
    named = [(n, torch.nn.Parameter(torch.randn(*s, generator=g))) for n, s in SHAPES]
    return FlatParams(named, lambda n: 'convs' in n)


def _state(rank=R, names=None, seed=0):
    from rick_amd.kml import KmlState
    flat = _flat(seed)
    return flat, KmlState(flat, rank, names=names, generator=torch.Generator().manual_seed(5))


def _rows(k, seed=3, p=0.5):
    rng = np.random.RandomState(seed)
    out = {}
    for n in k.names:
        f = rng.rand(k.shape3[n][0]) < p
        f[0] = True
        out[n] = torch.from_numpy(f)
    return out


def _fill(k, seed=9):
    """Non-trivial a on the flagged rows and a gradient in flat.grad."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n in k.names:
            k.a[n].copy_(0.3 * torch.randn(k.a[n].shape, generator=g) * k.rows[n][:, None])
        k.flat.grad.copy_(torch.randn(k.flat.grad.shape, generator=g))


def _np(t):
    return t.detach().cpu().numpy()


def test_default_names_layout_and_initial_values():
    flat, k = _state()
    assert k.names == DEFAULT and k.rank == R and (k.lo, k.hi) == (flat.lo, flat.hi)
    assert k.shape3 == {'convs.0.w': (6, 5, 9), 'convs.1.w': (7, 4, 9), 'convs.2.skip': (9, 8, 1)}
    assert k.w0.shape == (flat.hi - flat.lo,) and not k.w0.any()
    for n in k.names:
        assert k.a[n].shape == (k.shape3[n][0], R) and not k.a[n].any()
        assert k.b[n].shape == (k.shape3[n][1], R) and float(k.b[n].detach().std()) > 0.3
        assert not k.rows[n].any() and k.rows[n].dtype == torch.bool
        assert torch.equal(k.modulation(n), torch.ones(k.shape3[n][:2]))
        assert torch.equal(k.weight(n).reshape(-1), flat.params[flat.index[n]].detach().reshape(-1))
    # the generator decides b
    _, k2 = _state()
    assert all(torch.equal(k.b[n], k2.b[n]) for n in k.names)
    assert k.flagged == 0 and k.nblocks == 0
    # named explicitly: a 2-D weight has taps = 1
    _, k3 = _state(names=['convs.3.fc'])
    assert k3.shape3 == {'convs.3.fc': (5, 11, 1)}


def test_first_apply_returns_w0_bit_for_bit_and_touches_nothing_else():
    flat, k = _state()
    before = flat.flat.clone()
    k.set_rows(_rows(k))
    k.apply_()
    assert torch.equal(flat.flat, before)                      # a = 0: W0 (1 + 0)
    _fill(k)
    k.apply_()
    changed = flat.flat != before
    allowed = torch.zeros_like(changed)
    for n in k.names:
        lo, _ = flat.segment(n)
        co, ci, taps = k.shape3[n]
        for o in np.flatnonzero(_np(k.rows[n])):
            allowed[lo + o * ci * taps: lo + (o + 1) * ci * taps] = True
    assert bool(changed.any()) and not bool((changed & ~allowed).any())


def test_cpu_path_vs_fp64():
    flat, k = _state()
    k.set_rows(_rows(k))
    _fill(k)
    w0 = {n: _np(k.snapshot(n)).copy() for n in k.names}
    k.apply_()
    k.grads_()
    worst = [0.0, 0.0, 0.0]
    for n in k.names:
        rows = _np(k.rows[n])
        a, b, g = _np(k.a[n]), _np(k.b[n]), _np(k.grad(n))
        ref, bound = kml_f64.apply(w0[n], a, b), kml_f64.apply_bound(w0[n], a, b)
        err = np.abs(_np(k.weight(n)).astype(np.float64) - ref)[rows]
        assert (err <= bound[rows]).all(), n
        worst[0] = max(worst[0], float((err / np.maximum(bound[rows], 1e-300)).max()))
        da, db = kml_f64.grads(g, w0[n], a, b, rows)
        bda, bdb = kml_f64.grad_bounds(g, w0[n], a, b, rows)
        eda, edb = np.abs(_np(k.a[n].grad) - da), np.abs(_np(k.b[n].grad) - db)
        assert (eda <= bda).all() and (edb <= bdb).all(), n
        assert not _np(k.a[n].grad)[~rows].any() and np.abs(da[rows]).min() > 0
        worst[1] = max(worst[1], float((eda[rows] / bda[rows]).max()))
        worst[2] = max(worst[2], float((edb / np.maximum(bdb, 1e-300)).max()))
    print(f'kml cpu: error / bound  W^ {worst[0]:.3f}  da {worst[1]:.3f}  db {worst[2]:.3f}')


def test_grads_vs_autograd():
    flat, k = _state()
    k.set_rows(_rows(k))
    _fill(k)
    k.grads_()
    for n in k.names:
        rows = k.rows[n]
        a = k.a[n].detach().double().requires_grad_(True)
        b = k.b[n].detach().double().requires_grad_(True)
        w = k.snapshot(n).double() * (1 + a @ b.T)[..., None]
        (w[rows] * k.grad(n).double()[rows]).sum().backward()
        bda, bdb = kml_f64.grad_bounds(_np(k.grad(n)), _np(k.snapshot(n)), _np(a), _np(b), _np(rows))
        eda, edb = _np((k.a[n].grad - a.grad).abs()), _np((k.b[n].grad - b.grad).abs())
        print(f'kml autograd {n}: error / bound  da {float((eda / np.maximum(bda, 1e-300)).max()):.3f}  '
              f'db {float((edb / np.maximum(bdb, 1e-300)).max()):.3f}')
        assert (eda <= bda).all() and (edb <= bdb).all()


def test_set_rows_enter_leave_b_persists_moments_zeroed():
    flat, k = _state()
    n = 'convs.0.w'
    first = torch.tensor([True, True, False, False, True, False])
    live0 = k.weight(n).clone()
    k.set_rows({n: first})
    assert torch.equal(k.snapshot(n)[first], live0[first]) and not k.snapshot(n)[~first].any()
    assert k.flagged == 3 and all(not k.rows[m].any() for m in k.names if m != n)      # other names keep their flags
    _fill(k)
    k.apply_()
    ai = k.fac.index[f'a.{n}']
    lo = int(k.fac.offsets[ai])
    k.optim.m[lo:lo + 6 * R] = 1.0
    k.optim.v[lo:lo + 6 * R] = 2.0
    b_before, a_before, w_before, w0_before = k.b[n].detach().clone(), k.a[n].detach().clone(), k.weight(n).clone(), k.snapshot(n).clone()
    second = torch.tensor([True, False, True, False, True, True])              # 1 leaves; 2 and 5 enter; 0 and 4 stay
    k.set_rows({n: second})
    enter, stay, leave = second & ~first, second & first, first & ~second
    assert torch.equal(k.weight(n), w_before)                                  # nothing is written to a weight
    assert torch.equal(k.snapshot(n)[enter], w_before[enter]) and not k.a[n][enter].any()
    assert torch.equal(k.snapshot(n)[stay], w0_before[stay]) and torch.equal(k.a[n][stay], a_before[stay]) and bool(a_before[stay].any())
    assert not torch.equal(w_before[leave], w0_before[leave])                  # the row that left keeps its W^, not W0
    assert torch.equal(k.b[n], b_before)
    m, v = k.optim.m[lo:lo + 6 * R].view(6, R), k.optim.v[lo:lo + 6 * R].view(6, R)
    assert not m[enter].any() and not v[enter].any() and bool((m[~enter] == 1).all()) and bool((v[~enter] == 2).all())
    assert torch.equal(k.rows[n], second) and k.flagged == 4
    k.set_rows({m: torch.zeros_like(k.rows[m]) for m in k.names})
    assert k.flagged == 0 and k.nblocks == 0
    k.grads_()
    assert not k.fac.grad.any()


def test_state_dict_round_trip_is_in_place():
    flat, k = _state()
    k.set_rows(_rows(k))
    _fill(k)
    cover = torch.zeros(k.fac.total)                                           # the factors' own elements (the padding stays zero)
    for o, size in zip(k.fac.offsets, k.fac.sizes):
        cover[int(o):int(o) + size] = 1
    k.optim.m.copy_(torch.rand(k.optim.m.shape) * cover)
    k.optim.v.copy_(torch.rand(k.optim.v.shape) * cover)
    k.optim.steps[:] = [3] * len(k.optim.steps)
    sd = k.state_dict()
    assert set(sd) == {'steps'} | {f'{p}.{n}' for n in k.names for p in ('w0', 'rows', 'a', 'b', 'm.a', 'v.a', 'm.b', 'v.b')}
    assert sd['w0.convs.1.w'].shape == (1, 7, 4, 3, 3) and sd['a.convs.1.w'].shape == (7, R) and sd['b.convs.1.w'].shape == (4, R)
    _, k2 = _state(seed=1)
    ptrs = (k2.w0.data_ptr(), k2.fac.flat.data_ptr(), k2.optim.m.data_ptr(), k2.a['convs.0.w'].data_ptr())
    live = k2.flat.flat.clone()
    k2.load_state_dict(sd)
    assert ptrs == (k2.w0.data_ptr(), k2.fac.flat.data_ptr(), k2.optim.m.data_ptr(), k2.a['convs.0.w'].data_ptr())
    assert torch.equal(k2.flat.flat, live)                                     # the parameters are not written
    assert torch.equal(k2.w0, k.w0) and torch.equal(k2.fac.flat, k.fac.flat)
    assert torch.equal(k2.optim.m, k.optim.m) and torch.equal(k2.optim.v, k.optim.v) and k2.optim.steps == k.optim.steps
    assert all(torch.equal(k2.rows[n], k.rows[n]) for n in k.names) and k2.flagged == k.flagged and k2.nblocks == k.nblocks
    sd2 = k2.state_dict()
    assert all(torch.equal(sd[key], sd2[key]) for key in sd)
    # a bad entry: nothing live is touched
    snap = (k2.w0.clone(), k2.fac.flat.clone(), k2.optim.m.clone())
    for key, bad, exc in (('b.convs.2.skip', torch.zeros(8, R + 1), ValueError), ('rows.convs.0.w', torch.zeros(6), ValueError),
                          ('a.convs.0.w', torch.full((6, R), float('nan')), ValueError), ('w0.convs.1.w', torch.zeros(7, 4, 3, 3), ValueError),
                          ('steps', torch.zeros(2, dtype=torch.int64), ValueError), ('m.a.convs.0.w', None, KeyError)):
        broken = {kk: torch.zeros_like(v) for kk, v in sd.items()}
        if bad is None:
            del broken[key]
        else:
            broken[key] = bad
        with pytest.raises(exc, match=key.replace('.', r'\.')):
            k2.load_state_dict(broken)
        assert torch.equal(k2.w0, snap[0]) and torch.equal(k2.fac.flat, snap[1]) and torch.equal(k2.optim.m, snap[2])


def test_validation_errors():
    from rick_amd.kml import KmlState
    flat = _flat()
    for bad in (0, 9, -1, 2.0, True, None):
        with pytest.raises(ValueError, match='rank'):
            KmlState(flat, bad)
    with pytest.raises(KeyError, match='nope'):
        KmlState(flat, 2, names=['nope'])
    with pytest.raises(ValueError, match='head.w'):
        KmlState(flat, 2, names=['head.w'])                    # outside the optimised slice
    with pytest.raises(ValueError, match='twice'):
        KmlState(flat, 2, names=['convs.0.w', 'convs.0.w'])
    with pytest.raises(ValueError, match='two dims'):
        KmlState(flat, 2, names=['convs.0.b'])
    with pytest.raises(ValueError, match='no parameter'):
        KmlState(flat, 2, names=[])
    k = KmlState(flat, 2)
    with pytest.raises(KeyError, match='convs.3.fc'):
        k.set_rows({'convs.3.fc': torch.zeros(5, dtype=torch.bool)})
    with pytest.raises(ValueError, match='convs.0.w'):
        k.set_rows({'convs.0.w': torch.zeros(5, dtype=torch.bool)})
    with pytest.raises(ValueError, match='convs.0.w'):
        k.set_rows({'convs.0.w': torch.zeros(6)})
    good = torch.ones(7, dtype=torch.bool)
    with pytest.raises(ValueError, match='convs.0.w'):         # validated before anything is touched
        k.set_rows({'convs.1.w': good, 'convs.0.w': torch.zeros(6, 1, dtype=torch.bool)})
    assert k.flagged == 0 and not k.w0.any()


def test_trainer_config_checks():
    from rick_amd.train import TrainConfig
    assert TrainConfig().kml_rank == 0


# ---- trainer: construction and step order with a stand-in (what the trainer uses of an adapter, and nothing else) ---------------
class _StandInKml:
    built = []

    def __init__(self, flat, rank, names=None, generator=None, lr=None, betas=None):
        self.flat, self.rank, self.lr, self.betas, self.log = flat, rank, lr, betas, None
        _StandInKml.built.append(self)

    def grads_(self):
        self.log.append('grads_')

    def adam_step(self):
        self.log.append('adam_step')

    def apply_(self):
        self.log.append('apply_')


def _make(monkeypatch, **cfg):
    from rick_amd import kml
    from rick_amd.models import Discriminator, Generator
    from rick_amd.train import RickTrainer, TrainConfig
    monkeypatch.setattr(kml, 'KmlState', _StandInKml)
    del _StandInKml.built[:]
    torch.manual_seed(0)
    nets = [f(32, *a, channel_multiplier=1) for f, a in ((Generator, (512, 2)), (Discriminator, ())) * 2]
    return RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, **cfg), *nets)


def test_step_order(monkeypatch):
    tr = _make(monkeypatch, kml_rank=2)
    assert [k.flat for k in _StandInKml.built] == [tr.g_flat, tr.d_flat] and (tr.kml_g, tr.kml_d) == tuple(_StandInKml.built)
    assert (tr.kml_g.rank, tr.kml_g.lr, tr.kml_g.betas) == (2, tr.g_optim.lr, tr.g_optim.betas)
    assert (tr.kml_d.rank, tr.kml_d.lr, tr.kml_d.betas) == (2, tr.d_optim.lr, tr.d_optim.betas)
    assert tr.svd_g is None and tr.svd_d is None and tr.g_optim.mask is None
    with pytest.raises(RuntimeError, match='hipGraph replay with kernel modulation'):
        tr.enable_graphs(True)
    with pytest.raises(RuntimeError, match='graph=True step with kernel modulation'):
        tr._run('g', lambda: None, tr.g_flat, tr.g_optim)
    for flat, optim, mine, other in ((tr.g_flat, tr.g_optim, tr.kml_g, tr.kml_d), (tr.d_flat, tr.d_optim, tr.kml_d, tr.kml_g)):
        log, stray = [], []
        mine.log, other.log = log, stray
        monkeypatch.setattr(tr, '_reduce', lambda f, log=log: log.append(('reduce', f)))
        monkeypatch.setattr(optim, 'step', lambda log=log: log.append('optim.step'))
        tr._run(None, lambda log=log: log.append('fb'), flat, optim, pre=lambda log=log: log.append('pre'))
        assert log == ['pre', 'fb', ('reduce', flat), 'grads_', 'optim.step', 'adam_step', 'apply_'] and not stray
    # off: the step is the plain one
    tr = _make(monkeypatch)
    assert tr.kml_g is None and tr.kml_d is None and not _StandInKml.built
    log = []
    monkeypatch.setattr(tr.g_optim, 'step', lambda: log.append('optim.step'))
    tr._run(None, lambda: log.append('fb'), tr.g_flat, tr.g_optim)
    assert log == ['fb', 'optim.step']


def test_c_entries_reject_bad_arguments():
    """RICK_EINVAL (22) from every entry, before any launch: no GPU involved."""
    import ctypes

    from rick_amd._lib import KmlLayer, lib
    assert ctypes.sizeof(KmlLayer) == 64
    assert lib.rick_kml_rows_per_group(512, 9) == 4 and lib.rick_kml_rows_per_group(512, 1) == 32
    assert lib.rick_kml_rows_per_group(1, 1) == 64 and lib.rick_kml_rows_per_group(0, 9) == -1 and lib.rick_kml_rows_per_group(8, 0) == -1
    p = 4096                                                   # a fake, aligned, non-null address: never dereferenced
    ok_apply = [p, 2 * p, 100, 3 * p, 100, 2, 4 * p, 1, 5 * p, 1, 6 * p, 1, None]
    ok_grad = [p, 2 * p, 100, 3 * p, 7 * p, 100, 8 * p, 100, 2, 4 * p, 1, 5 * p, 1, 6 * p, 1, 64, None]
    ok_fin = [8 * p, 100, 7 * p, 100, 9 * p, 10, 2, 4 * p, 1, 8, 8, None]

    def bad(fn, args, pos, val):
        a = list(args)
        a[pos] = val
        return fn(*a)
    for pos, val in ((0, None), (1, None), (1, p), (0, p + 2), (2, -1), (3, None), (4, -1), (5, 0), (5, 9), (6, None), (6, 4 * p + 4),
                     (7, 0), (8, None), (9, -1), (10, None), (11, -1)):
        assert bad(lib.rick_kml_apply_f32, ok_apply, pos, val) == 22, ('apply', pos, val)
    for pos, val in ((0, None), (1, None), (2, -1), (3, None), (4, None), (4, 3 * p), (5, -1), (6, None), (7, -1), (8, 0), (8, 9),
                     (9, None), (10, 0), (11, None), (12, -1), (13, None), (14, -1), (15, 0), (15, 40000)):
        assert bad(lib.rick_kml_grad_f32, ok_grad, pos, val) == 22, ('grad', pos, val)
    for pos, val in ((0, None), (1, -1), (2, None), (3, -1), (4, None), (5, -1), (6, 0), (6, 9), (7, None), (8, 0), (9, 0), (10, 0)):
        assert bad(lib.rick_kml_grad_finish_f32, ok_fin, pos, val) == 22, ('finish', pos, val)
    # nothing flagged: apply and grad launch nothing and succeed
    assert bad(lib.rick_kml_apply_f32, ok_apply, 11, 0) == 0
    assert bad(lib.rick_kml_grad_f32, ok_grad, 14, 0) == 0
