"""rick_amd.svd on the CPU: the torch fp64 composition of apply_ / grads_ against the literal loops of tests/svd_f64.py, what the
construction stores, the freeze mask, the in-place state_dict round trip, the C ABI's refusals on the cross-built library and the
trainer's validation and step order (stand-in forwards and adapters: no decomposition, no device).  CPU-only; the kernels and the
real trainer run in tests/test_gpu_svd.py."""
import ctypes

import numpy as np
import pytest
import torch

from tests import svd_f64

EINVAL = 22
# registration order: outside the slice, co > ci, a bias, the generator's 5-D weight with co < ci, a 1x1 skip, a 2-D weight, co = 1
SHAPES = [('head.w', (4, 3, 3, 3)), ('convs.0.w', (6, 5, 3, 3)), ('convs.0.b', (6,)), ('convs.1.w', (1, 4, 7, 3, 3)),
          ('convs.2.skip', (9, 8, 1, 1)), ('convs.3.fc', (5, 11)), ('convs.4.out', (1, 6)), ('tail.w', (7,))]
ADAPTED = ['convs.0.w', 'convs.1.w', 'convs.2.skip', 'convs.3.fc', 'convs.4.out']


def _flat(seed=0):
    from rick_amd.train import FlatParams
    g = torch.Generator().manual_seed(seed)
    named = [(n, torch.nn.Parameter(torch.randn(*s, generator=g))) for n, s in SHAPES]
    return FlatParams(named, lambda n: 'convs' in n)


def _adapter(seed=0, names=None):
    from rick_amd.svd import SvdAdapter
    flat = _flat(seed)
    return flat, SvdAdapter(flat, names=names)


def _fill(a, seed=9):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n in a.names:
            a.d[n].copy_(0.1 * a.s0[n] * torch.randn(a.d[n].shape, generator=g))
        a.flat.grad.copy_(torch.randn(a.flat.grad.shape, generator=g))


def _np(t):
    return t.detach().cpu().numpy()


def test_f64_forms_agree():
    rng = np.random.RandomState(0)
    for co, ci, taps in ((3, 5, 2), (6, 4, 3), (1, 7, 1)):
        r = min(co, ci)
        w0, g = rng.standard_normal((co, ci, taps)), rng.standard_normal((co, ci, taps))
        u, vt, d = rng.standard_normal((taps, co, r)), rng.standard_normal((taps, r, ci)), rng.standard_normal((taps, r))
        a, b = svd_f64.apply_loops(w0, u, vt, d), svd_f64.apply(w0, u, vt, d)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
        a, b = svd_f64.grad_loops(g, u, vt), svd_f64.grad(g, u, vt)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


def test_torch_composition_agrees_with_the_loops():
    """rick_amd.svd.compose_apply / compose_grad (what CPU tensors take, in fp64) against the literal loops, to 1e-12."""
    from rick_amd.svd import compose_apply, compose_grad
    rng = np.random.RandomState(1)
    for co, ci, taps in ((3, 5, 2), (6, 4, 9), (1, 7, 1), (5, 1, 3)):
        r = min(co, ci)
        w0, g = rng.standard_normal((co, ci, taps)).astype(np.float32), rng.standard_normal((co, ci, taps)).astype(np.float32)
        u, vt = rng.standard_normal((taps, co, r)).astype(np.float32), rng.standard_normal((taps, r, ci)).astype(np.float32)
        d = rng.standard_normal((taps, r)).astype(np.float32)
        tw0, tg, tu, tvt, td = (torch.from_numpy(x) for x in (w0, g, u, vt, d))
        got, ref = compose_apply(tw0, tu, tvt, td), svd_f64.apply_loops(w0, u, vt, d)
        assert got.dtype == torch.float64 and got.shape == (co, ci, taps) and np.abs(got.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()
        got, ref = compose_grad(tg, tu, tvt), svd_f64.grad_loops(g, u, vt)
        assert got.dtype == torch.float64 and got.shape == (taps, r) and np.abs(got.numpy() - ref).max() <= 1e-12 * np.abs(ref).max()


def test_default_names_shapes_and_construction():
    flat, a = _adapter()
    assert a.names == ADAPTED and (a.lo, a.hi) == (flat.lo, flat.hi)
    assert a.shape3 == {'convs.0.w': (6, 5, 9), 'convs.1.w': (4, 7, 9), 'convs.2.skip': (9, 8, 1), 'convs.3.fc': (5, 11, 1),
                        'convs.4.out': (1, 6, 1)}
    assert a.rank == {'convs.0.w': 5, 'convs.1.w': 4, 'convs.2.skip': 8, 'convs.3.fc': 5, 'convs.4.out': 1}      # co > ci, co < ci, co = 1
    assert torch.equal(a.w0, flat.flat[flat.lo:flat.hi]) and a.w0.data_ptr() != flat.flat[flat.lo:].data_ptr()
    for n in a.names:
        co, ci, taps = a.shape3[n]
        r = a.rank[n]
        assert a.u[n].shape == (taps, co, r) and a.vt[n].shape == (taps, r, ci) and a.s0[n].shape == (taps, r) == a.d[n].shape
        assert a.u[n].dtype == a.vt[n].dtype == torch.float32 and not a.d[n].any()
        assert bool((a.s0[n][:, :-1] >= a.s0[n][:, 1:]).all()) and bool((a.s0[n] >= 0).all())
        # U diag(s0) Vt rebuilds W0 to fp32 round-off: three fp32 roundings of factors of a sum of r terms
        re = torch.bmm(a.u[n].double() * a.s0[n].double()[:, None, :], a.vt[n].double()).permute(1, 2, 0)
        err = float((re - a.snapshot(n).double()).abs().max() / a.snapshot(n).abs().max())
        assert err <= (r + 3) * 2.0 ** -23, (n, err)
        # the stored factors against the host decomposition, and near-orthogonality as stored
        eye = torch.bmm(a.u[n].double().transpose(1, 2), a.u[n].double()) - torch.eye(r, dtype=torch.float64)
        assert float(eye.abs().max()) < 1e-6
        assert torch.equal(a.singular_values(n), a.s0[n])
    _, b = _adapter(names=['convs.3.fc'])
    assert b.names == ['convs.3.fc'] and b.tables.nlayers == 1


def test_zero_shift_returns_w0_exactly_and_touches_nothing_else():
    flat, a = _adapter()
    before = flat.flat.clone()
    with torch.no_grad():
        flat.flat[flat.lo:flat.hi] += 1.0                      # the live weights have drifted: apply_ re-imposes W0
    drifted = flat.flat.clone()
    a.apply_()
    adapted = a.frozen_mask(rest=True).bool()
    assert torch.equal(flat.flat[adapted], before[adapted]) and torch.equal(flat.flat[~adapted], drifted[~adapted])


def test_cpu_path_vs_fp64_loops():
    flat, a = _adapter()
    _fill(a)
    a.apply_()
    a.grads_()
    for n in a.names:
        u, vt, d = _np(a.u[n]), _np(a.vt[n]), _np(a.d[n])
        ref = svd_f64.apply_loops(_np(a.snapshot(n)), u, vt, d)
        # the composition is fp64 rounded once to fp32
        assert np.abs(_np(a.weight(n)) - ref).max() <= 2.0 ** -24 * np.abs(ref).max() * 1.0000001
        assert not np.array_equal(_np(a.weight(n)), _np(a.snapshot(n)))
        ref = svd_f64.grad_loops(_np(a.grad(n)), u, vt)
        assert np.abs(_np(a.d[n].grad) - ref).max() <= 2.0 ** -24 * np.abs(ref).max() * 1.0000001
        # and against autograd through the definition
        dd = a.d[n].detach().double().requires_grad_(True)
        w = a.snapshot(n).double() + torch.bmm(a.u[n].double() * dd[:, None, :], a.vt[n].double()).permute(1, 2, 0)
        (w * a.grad(n).double()).sum().backward()
        assert float((dd.grad - torch.from_numpy(ref)).abs().max()) <= 1e-12 * np.abs(ref).max()
        assert torch.equal(a.singular_values(n), a.s0[n] + a.d[n].detach())


def test_frozen_mask_bits():
    flat, a = _adapter()
    for rest in (False, True):
        m = a.frozen_mask(rest=rest)
        assert m.dtype == torch.uint8 and m.shape == (flat.total,) and int(m.max()) == 1
        for n, _ in SHAPES:
            lo, hi = flat.segment(n)
            want = n in ADAPTED or (not rest and flat.lo <= lo < flat.hi)
            assert bool((m[lo:hi] == int(want)).all()), (n, rest)
        assert not m[:flat.lo].any() and not m[flat.hi:].any()
    _, b = _adapter(names=['convs.0.w'])
    lo, hi = b.flat.segment('convs.1.w')
    assert not b.frozen_mask(rest=True)[lo:hi].any() and bool(b.frozen_mask()[lo:hi].all())


def test_state_dict_round_trip_is_in_place():
    flat, a = _adapter()
    _fill(a)
    cover = torch.zeros(a.fac.total)
    for o, size in zip(a.fac.offsets, a.fac.sizes):
        cover[int(o):int(o) + size] = 1
    a.optim.m.copy_(torch.rand(a.optim.m.shape) * cover)
    a.optim.v.copy_(torch.rand(a.optim.v.shape) * cover)
    a.optim.steps[:] = [3] * len(a.optim.steps)
    sd = a.state_dict()
    assert set(sd) == {'steps'} | {f'{p}.{n}' for n in a.names for p in ('w0', 'u', 'vt', 's0', 'd', 'm.d', 'v.d')}
    assert sd['w0.convs.1.w'].shape == (1, 4, 7, 3, 3) and sd['u.convs.1.w'].shape == (9, 4, 4) and sd['vt.convs.1.w'].shape == (9, 4, 7)
    assert sd['d.convs.1.w'].shape == (9, 4) and sd['u.convs.0.w'].data_ptr() != a.u['convs.0.w'].data_ptr()
    _, b = _adapter(seed=1)
    ptrs = (b.w0.data_ptr(), b.u_flat.data_ptr(), b.vt_flat.data_ptr(), b.fac.flat.data_ptr(), b.optim.m.data_ptr(), b.d['convs.0.w'].data_ptr())
    live = b.flat.flat.clone()
    b.load_state_dict(sd)
    assert ptrs == (b.w0.data_ptr(), b.u_flat.data_ptr(), b.vt_flat.data_ptr(), b.fac.flat.data_ptr(), b.optim.m.data_ptr(),
                    b.d['convs.0.w'].data_ptr())
    assert torch.equal(b.flat.flat, live)                      # the parameters are not written
    for n in a.names:
        assert torch.equal(b.snapshot(n), a.snapshot(n)) and torch.equal(b.u[n], a.u[n]) and torch.equal(b.vt[n], a.vt[n])
        assert torch.equal(b.d[n], a.d[n]) and torch.equal(b.s0[n], a.s0[n])
    assert torch.equal(b.optim.m, a.optim.m) and torch.equal(b.optim.v, a.optim.v) and b.optim.steps == a.optim.steps
    sd2 = b.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    # a bad entry: rejected before anything live is touched
    snap = (b.w0.clone(), b.u_flat.clone(), b.vt_flat.clone(), b.fac.flat.clone(), b.optim.m.clone())
    for key, bad, exc in (('vt.convs.2.skip', torch.zeros(1, 8, 9), ValueError), ('u.convs.0.w', torch.zeros(9, 6, 6), ValueError),
                          ('d.convs.0.w', torch.full((9, 5), float('nan')), ValueError), ('w0.convs.1.w', torch.zeros(4, 7, 3, 3), ValueError),
                          ('d.convs.3.fc', torch.zeros(1, 5, dtype=torch.float64), ValueError),
                          ('steps', torch.zeros(2, dtype=torch.int64), ValueError), ('m.d.convs.4.out', None, KeyError)):
        broken = {kk: torch.zeros_like(v) for kk, v in sd.items()}
        if bad is None:
            del broken[key]
        else:
            broken[key] = bad
        with pytest.raises(exc, match=key.replace('.', r'\.')):
            b.load_state_dict(broken)
        now = (b.w0, b.u_flat, b.vt_flat, b.fac.flat, b.optim.m)
        assert all(torch.equal(x, y) for x, y in zip(now, snap)) and b.optim.steps == [3] * len(b.optim.steps)


def test_validation_errors():
    from rick_amd.svd import SvdAdapter
    flat = _flat()
    with pytest.raises(KeyError, match='nope'):
        SvdAdapter(flat, names=['nope'])
    with pytest.raises(ValueError, match='head.w'):
        SvdAdapter(flat, names=['head.w'])                     # outside the optimised slice
    with pytest.raises(ValueError, match='twice'):
        SvdAdapter(flat, names=['convs.0.w', 'convs.0.w'])
    with pytest.raises(ValueError, match='svd: .*two dims'):
        SvdAdapter(flat, names=['convs.0.b'])
    with pytest.raises(ValueError, match='no parameter'):
        SvdAdapter(flat, names=[])


# ---- C ABI on the cross-built library: every refusal comes before any launch, no device involved ------------------------------
def _table(*recs):
    from rick_amd._lib import SvdLayer
    t = (SvdLayer * len(recs))()
    for L, (off, u_off, vt_off, d_off, part_off, co, ci, taps, r) in zip(t, recs):
        L.off, L.u_off, L.vt_off, L.d_off, L.part_off, L.co, L.ci, L.taps, L.r = off, u_off, vt_off, d_off, part_off, co, ci, taps, r
    return t


def test_c_entries_reject_bad_arguments():
    from rick_amd._lib import SvdLayer, lib
    assert ctypes.sizeof(SvdLayer) == 64
    # tiles: 32 rows x 32 s columns (apply), 32 s directions x 32 columns (grad); s = 1, 2, 4 for taps >= 3, 2, 1
    assert lib.rick_svd_apply_tiles(512, 512, 9) == 256 and lib.rick_svd_apply_tiles(512, 8192, 1) == 16 * 64
    assert lib.rick_svd_apply_tiles(33, 70, 9) == 2 * 3 and lib.rick_svd_apply_tiles(1, 512, 1) == 4 and lib.rick_svd_apply_tiles(5, 65, 2) == 2
    assert lib.rick_svd_grad_tiles(512, 512, 9) == 256 and lib.rick_svd_grad_tiles(1, 512, 1) == 16 and lib.rick_svd_grad_tiles(130, 40, 1) == 2
    assert lib.rick_svd_partials(33, 70, 9) == 9 * 33 * 3 and lib.rick_svd_partials(70, 33, 9) == 9 * 33 * 2
    for fn in (lib.rick_svd_apply_tiles, lib.rick_svd_grad_tiles, lib.rick_svd_partials):
        assert fn(0, 4, 1) == -1 and fn(4, 0, 1) == -1 and fn(4, 4, 0) == -1 and fn(4, 4, 17) == -1
    # (33, 70, 9) at 5 and (3, 32, 1) behind it
    n1, u1, v1, d1, p1 = 33 * 70 * 9, 9 * 33 * 33, 9 * 33 * 70, 9 * 33, 9 * 33 * 3
    good = [(5, 0, 0, 0, 0, 33, 70, 9, 33), (5 + n1 + 2, u1, v1, 64 * 5, p1, 3, 32, 1, 3)]
    n, nu, nvt, nd, npart = 5 + n1 + 2 + 96, u1 + 9, v1 + 96, 64 * 5 + 3, p1 + 3

    def check(recs, *lens):
        t = _table(*recs)
        return lib.rick_svd_check_table(ctypes.addressof(t), len(recs), *lens)
    assert check(good, n, nu, nvt, nd, npart) == 0
    for k, short in enumerate((n - 1, nu - 1, nvt - 1, nd - 1, npart - 1)):                    # an extent past each buffer in turn
        lens = [n, nu, nvt, nd, npart]
        lens[k] = short
        assert check(good, *lens) == EINVAL, k
        lens[k] = -1
        assert check(good, *lens) == EINVAL, k
    for pos, val in ((8, 32), (8, 70), (8, 0), (5, 0), (6, -1), (7, 0), (7, 17), (0, -1), (1, -4), (2, -1), (3, -1), (4, -1), (0, n)):
        rec = list(good[0])
        rec[pos] = val
        assert check([tuple(rec), good[1]], n, nu, nvt, nd, npart) == EINVAL, (pos, val)      # r != min(co, ci), bad shape, bad offset
    assert lib.rick_svd_check_table(None, 2, n, nu, nvt, nd, npart) == EINVAL
    assert check(good[:1], n, nu, nvt, nd, npart) == 0
    # the entries: host memory everywhere (this is what a CPU tensor's data_ptr() is) with a good table is refused, and so is
    # every null / misaligned pointer, a bad table and a block count that is not the table's tile count
    t = _table(*good)
    th = ctypes.addressof(t)
    buf = (ctypes.c_float * (8 * n))()
    p = ctypes.addressof(buf)
    w0, w, u, vt, d, blocks = p, p + 4 * n, p + 8 * n, p + 12 * n, p + 16 * n, p + 20 * n
    na, ng = 6 + 1, 6 + 1
    ok_apply = [w0, w, n, u, nu, vt, nvt, d, nd, th, th, 2, blocks, na, None]
    ok_grad = [w0, n, u, nu, vt, nvt, w, npart, th, th, 2, blocks, ng, None]
    ok_fin = [w, npart, d, nd, th, th, 2, None]
    assert lib.rick_svd_apply_f32(*ok_apply) == EINVAL and lib.rick_svd_grad_f32(*ok_grad) == EINVAL      # CPU pointers
    assert lib.rick_svd_grad_finish_f32(*ok_fin) == EINVAL

    def bad(fn, args, pos, val):
        a = list(args)
        a[pos] = val
        return fn(*a)
    bad_table = _table((5, 0, 0, 0, 0, 33, 70, 9, 32), good[1])
    bad_t = ctypes.addressof(bad_table)
    for pos, val in ((0, None), (1, None), (1, w0), (0, w0 + 2), (2, n - 1), (3, None), (4, nu - 1), (5, None), (6, nvt - 1), (7, None),
                     (8, nd - 1), (9, None), (10, None), (10, bad_t), (11, 0), (12, None), (13, na + 1), (13, 0)):
        assert bad(lib.rick_svd_apply_f32, ok_apply, pos, val) == EINVAL, ('apply', pos, val)
    for pos, val in ((0, None), (1, n - 1), (2, None), (3, nu - 1), (4, None), (5, nvt - 1), (6, None), (7, npart - 1), (8, None),
                     (9, None), (9, bad_t), (10, 0), (11, None), (12, ng - 1)):
        assert bad(lib.rick_svd_grad_f32, ok_grad, pos, val) == EINVAL, ('grad', pos, val)
    for pos, val in ((0, None), (1, npart - 1), (2, None), (3, nd - 1), (4, None), (5, None), (5, bad_t), (6, 0)):
        assert bad(lib.rick_svd_grad_finish_f32, ok_fin, pos, val) == EINVAL, ('finish', pos, val)


def test_tables_and_raw_entries_on_the_host():
    from rick_amd.svd import SvdTables, apply_tables
    t = SvdTables([dict(off=5, u_off=0, vt_off=0, d_off=0, shape=(33, 70, 9)), dict(off=30000, u_off=9801, vt_off=20790, d_off=320, shape=(1, 512, 1))],
                  'cpu')
    assert (t.nlayers, t.n_apply, t.n_grad, t.npart) == (2, 6 + 4, 6 + 16, 9 * 33 * 3 + 16)
    assert t.flops == 2 * 33 * 70 * 9 * 33 + 2 * 512 and t.layers_host[1].part_off == 9 * 33 * 3 and t.layers_host[1].r == 1
    with pytest.raises(ValueError, match='taps'):
        SvdTables([dict(off=0, u_off=0, vt_off=0, d_off=0, shape=(4, 4, 25))], 'cpu')
    x = torch.zeros(8)
    with pytest.raises(ValueError, match='HIP device'):         # CPU tensors never reach the library
        apply_tables(x, x.clone(), x, x, x, t)


# ---- trainer: validation and step order with stand-ins -----------------------------------------------------------------------
class _StandInAdapter:
    built = []

    def __init__(self, flat, names=None, lr=None, betas=None):
        self.flat, self.lr, self.betas, self.log = flat, lr, betas, None
        _StandInAdapter.built.append(self)

    def frozen_mask(self, rest=False):
        self.rest = rest
        return torch.full((self.flat.total,), 1 if not rest else 0, dtype=torch.uint8)

    def grads_(self):
        self.log.append('grads_')

    def adam_step(self):
        self.log.append('adam_step')

    def apply_(self):
        self.log.append('apply_')


def _make(monkeypatch, **cfg):
    from rick_amd import svd
    from rick_amd.models import Discriminator, Generator
    from rick_amd.train import RickTrainer, TrainConfig
    monkeypatch.setattr(svd, 'SvdAdapter', _StandInAdapter)
    del _StandInAdapter.built[:]
    torch.manual_seed(0)
    nets = [f(32, *a, channel_multiplier=1) for f, a in ((Generator, (512, 2)), (Discriminator, ())) * 2]
    return RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, **cfg), *nets)


def test_config_defaults_are_off():
    from rick_amd.train import TrainConfig
    assert TrainConfig().svd_adapt is False and TrainConfig().svd_train_rest is False


def test_trainer_validation_and_construction(monkeypatch):
    with pytest.raises(ValueError, match='kml_rank'):
        _make(monkeypatch, svd_adapt=True, warmup_iter=0, kml_rank=2)
    with pytest.raises(ValueError, match='warmup_iter'):
        _make(monkeypatch, svd_adapt=True, warmup_iter=250)
    tr = _make(monkeypatch, warmup_iter=0)
    assert tr.svd_g is None and tr.svd_d is None and not _StandInAdapter.built and tr.g_optim.mask is None
    tr.enable_graphs(False)
    for rest in (False, True):
        tr = _make(monkeypatch, svd_adapt=True, svd_train_rest=rest, warmup_iter=0)
        assert [a.flat for a in _StandInAdapter.built] == [tr.g_flat, tr.d_flat] and (tr.svd_g, tr.svd_d) == tuple(_StandInAdapter.built)
        assert (tr.svd_g.lr, tr.svd_g.betas) == (tr.g_optim.lr, tr.g_optim.betas) and (tr.svd_d.lr, tr.svd_d.betas) == (tr.d_optim.lr, tr.d_optim.betas)
        assert tr.svd_g.rest is rest and tr.svd_d.rest is rest
        assert tr.g_optim.mask.shape == (tr.g_flat.total,) and bool((tr.g_optim.mask == (0 if rest else 1)).all())
        assert tr.d_optim.mask.shape == (tr.d_flat.total,)
    with pytest.raises(RuntimeError, match='hipGraph replay with singular-value adaptation'):
        tr.enable_graphs(True)
    with pytest.raises(RuntimeError, match='graph=True step with singular-value adaptation'):
        tr._run('g', lambda: None, tr.g_flat, tr.g_optim)
    with pytest.raises(RuntimeError, match='fisher_sweep'):
        tr.fisher_sweep([], [], first=True)
    with pytest.raises(RuntimeError, match='fisher_inputs'):
        tr.iteration(0, None, fisher_inputs=([], []))


def test_step_order(monkeypatch):
    tr = _make(monkeypatch, svd_adapt=True, warmup_iter=0)
    for flat, optim, mine, other in ((tr.g_flat, tr.g_optim, tr.svd_g, tr.svd_d), (tr.d_flat, tr.d_optim, tr.svd_d, tr.svd_g)):
        log = mine.log = other.log = []
        monkeypatch.setattr(tr, '_reduce', lambda f, log=log: log.append(('reduce', f)))
        monkeypatch.setattr(optim, 'step', lambda log=log: log.append('optim.step'))
        tr._run(None, lambda log=log: log.append('fb'), flat, optim, pre=lambda log=log: log.append('pre'))
        assert log == ['pre', 'fb', ('reduce', flat), 'grads_', 'optim.step', 'adam_step', 'apply_']
    # off: the step is the plain one
    tr = _make(monkeypatch, warmup_iter=0)
    log = []
    monkeypatch.setattr(tr.g_optim, 'step', lambda: log.append('optim.step'))
    tr._run(None, lambda: log.append('fb'), tr.g_flat, tr.g_optim)
    assert log == ['fb', 'optim.step']
