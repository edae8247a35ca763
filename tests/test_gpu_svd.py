"""rick_svd_apply_f32 / rick_svd_grad_f32 / rick_svd_grad_finish_f32 (rick_amd/csrc/svd.hip) and everything rick_amd/svd.py and the
trainer build on them, against the fp64 restatement tests/svd_f64.py.

Parity (the project's fourfold rule): W^ is measured over the max-norm of the reference W^, dd over the max-norm of the reference
dd.  The BASE is the error of the plain fp32 torch CPU composition of the same definition (permuted copies + torch.bmm) against
the same fp64 reference on the same inputs, measured here; the device is held to 4 x base.  Where the base itself sits at
round-off (r = 1 or 3: no summation error to quadruple) the bound has the floor 4 * 2^-23 of the max-norm.  Every test prints base,
device figure and bound (run with -s).

Inputs: weights N(0, 1), U and Vt from torch.linalg.svd in fp64 rounded to fp32 (real decompositions), d = 0.1 s0 N(0, 1),
G ~ N(0, 1).  The reference of a shape is computed once and shared; that of (512, 512, 9) — 4608 (t, k) passes over a 512 x 512 fp64
array in each direction — takes most of that case's 15 s on the host, the launches themselves under a millisecond.

The trainer tests hold every adapted layer to the fp64 torch composition (which tests/test_svd.py holds to svd_f64's loops at
1e-12) and a few layers — a linear weight, a 1 x 1 skip, [1, 512] and one 512 x 512 x 9 convolution — to svd_f64 itself: its loops
over (t, k) cost seconds per 512 x 512 x 9 layer, and a 32 px network has thirteen of them."""
import numpy as np
import pytest
import torch

from tests import svd_f64

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FLOOR = 4 * 2.0 ** -23

# (co, ci, taps): r = 3 either way round; co = 1; ragged in every dimension with r = 33, both ways round; full tiles; taps = 1 with
# more rows than a tile and a ragged 128-column tile; many tiles and a long K
SHAPES = [(3, 32, 1), (32, 3, 9), (1, 512, 1), (33, 70, 9), (70, 33, 9), (64, 64, 9), (130, 40, 1), (512, 512, 9)]
TABLE = [(33, 70, 9), (1, 512, 1), (70, 33, 9), (130, 40, 1), (32, 3, 9)]
_cache = {}


def _bases(w0, g, u, vt, d):
    """(fp64 W^, fp64 dd, base of W^, base of dd): the references and the relative max-norm error of the fp32 torch CPU composition."""
    ref_w, ref_d = svd_f64.apply(w0, u, vt, d), svd_f64.grad(g, u, vt)
    tw0, tg, tu, tvt, td = (torch.from_numpy(np.ascontiguousarray(x)) for x in (w0, g, u, vt, d))
    cw = tw0 + torch.bmm(tu * td[:, None, :], tvt).permute(1, 2, 0)
    cd = (torch.bmm(tu.transpose(1, 2).contiguous(), tg.permute(2, 0, 1).contiguous()) * tvt).sum(2)
    bw = float(np.abs(cw.numpy().astype(np.float64) - ref_w).max() / np.abs(ref_w).max())
    bd = float(np.abs(cd.numpy().astype(np.float64) - ref_d).max() / np.abs(ref_d).max())
    return ref_w, ref_d, bw, bd


def _layer(shape):
    """W0, G, U, Vt, d, s0 of one layer (NumPy fp32) with the fp64 references and the fp32 bases: computed once, never written."""
    if shape not in _cache:
        co, ci, taps = shape
        rng = np.random.RandomState(co * 1000 + ci * 10 + taps)
        w0 = rng.standard_normal(shape).astype(np.float32)
        U, S, Vh = torch.linalg.svd(torch.from_numpy(w0).double().permute(2, 0, 1).contiguous(), full_matrices=False)
        u, s0, vt = U.float().numpy(), S.float().numpy(), Vh.float().numpy()
        d = (0.1 * s0 * rng.standard_normal(s0.shape)).astype(np.float32)
        g = rng.standard_normal(shape).astype(np.float32)
        ref_w, ref_d, bw, bd = _bases(w0, g, u, vt, d)
        _cache[shape] = dict(w0=w0, g=g, u=u, vt=vt, d=d, s0=s0, ref_w=ref_w, ref_d=ref_d, base_w=bw, base_d=bd)
        for v in _cache[shape].values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _cache[shape]


class _Net:
    """Layers laid out in flat buffers: layer k of w / w0 / grad starts `phase[k]` floats past a 16-byte boundary, NaN in every gap
    of every buffer (w, w0, grad, u, vt, d)."""

    def __init__(self, shapes, phases=None):
        self.shapes = shapes
        self.data = [_layer(s) for s in shapes]
        phases = phases or [0] * len(shapes)
        self.woff, self.uoff, self.vtoff, self.doff = [], [], [], []
        pos = {'w': 4, 'u': 1, 'vt': 2, 'd': 3}
        for s, ph in zip(shapes, phases):
            co, ci, taps = s
            r = min(co, ci)
            pos['w'] = (pos['w'] + 3) // 4 * 4 + ph
            for key, lst, size in (('w', self.woff, co * ci * taps), ('u', self.uoff, taps * co * r), ('vt', self.vtoff, taps * r * ci),
                                   ('d', self.doff, taps * r)):
                lst.append(pos[key])
                pos[key] += size + 3
        self.n, self.nu, self.nvt, self.nd = (pos[k] + 2 for k in ('w', 'u', 'vt', 'd'))
        nan = lambda n: np.full(n, np.nan, dtype=np.float32)      # noqa: E731
        host = dict(w0=nan(self.n), g=nan(self.n), u=nan(self.nu), vt=nan(self.nvt), d=nan(self.nd))
        self.wmask, self.dmask = np.zeros(self.n, dtype=bool), np.zeros(self.nd, dtype=bool)
        for dat, wo, uo, vo, do in zip(self.data, self.woff, self.uoff, self.vtoff, self.doff):
            for key, off in (('w0', wo), ('g', wo), ('u', uo), ('vt', vo), ('d', do)):
                host[key][off:off + dat[key].size] = dat[key].reshape(-1)
            self.wmask[wo:wo + dat['w0'].size] = True
            self.dmask[do:do + dat['d'].size] = True
        self.host = host
        self.dev = {k: self._dev(v) for k, v in host.items()}
        from rick_amd.svd import SvdTables
        self.tables = SvdTables([dict(off=wo, u_off=uo, vt_off=vo, d_off=do, shape=s)
                                 for s, wo, uo, vo, do in zip(shapes, self.woff, self.uoff, self.vtoff, self.doff)], DEV)

    @staticmethod
    def _dev(x):
        t = torch.from_numpy(x).to(DEV)
        assert t.data_ptr() % 16 == 0
        return t

    def run(self, d=None, g=None):
        """apply into a buffer of NaN gaps and 7.0 on the adapted elements, grad into NaN; returns (w, dd) as NumPy and checks
        containment: the gaps of w are still NaN, no adapted element is, every dd is finite and the gaps of dd are untouched."""
        from rick_amd.svd import apply_tables, grad_tables
        w = self._dev(np.where(self.wmask, np.float32(7.0), np.float32(np.nan)).astype(np.float32))
        dd = self._dev(np.full(self.nd, np.nan, dtype=np.float32))
        partials = torch.full((self.tables.npart + 3,), float('nan'), device=DEV)
        apply_tables(self.dev['w0'], w, self.dev['u'], self.dev['vt'], self.dev['d'] if d is None else d, self.tables)
        grad_tables(self.dev['g'] if g is None else g, self.dev['u'], self.dev['vt'], dd, partials, self.tables)
        torch.cuda.synchronize()
        w, dd = w.cpu().numpy(), dd.cpu().numpy()
        assert np.isnan(w[~self.wmask]).all() and not np.isnan(w[self.wmask]).any()
        assert np.isfinite(dd[self.dmask]).all() and np.isnan(dd[~self.dmask]).all()
        assert bool(torch.isnan(partials[self.tables.npart:]).all())
        return w, dd

    def layer_w(self, w, k):
        return w[self.woff[k]:self.woff[k] + self.data[k]['w0'].size].reshape(self.shapes[k])

    def layer_d(self, dd, k):
        return dd[self.doff[k]:self.doff[k] + self.data[k]['d'].size].reshape(self.data[k]['d'].shape)


_nets = {}


def _single(shape):
    if shape not in _nets:
        net = _Net([shape])
        _nets[shape] = (net,) + net.run()
    return _nets[shape]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_parity_with_fp64(shape):
    net, w, dd = _single(shape)
    dat = net.data[0]
    ew = float(np.abs(net.layer_w(w, 0).astype(np.float64) - dat['ref_w']).max() / np.abs(dat['ref_w']).max())
    ed = float(np.abs(net.layer_d(dd, 0).astype(np.float64) - dat['ref_d']).max() / np.abs(dat['ref_d']).max())
    bw, bd = max(4 * dat['base_w'], FLOOR), max(4 * dat['base_d'], FLOOR)
    print(f"svd {shape}: W^ base {dat['base_w']:.3e} device {ew:.3e} bound {bw:.3e}   dd base {dat['base_d']:.3e} device {ed:.3e} bound {bd:.3e}")
    assert ew <= bw and ed <= bd
    assert not np.array_equal(net.layer_w(w, 0), dat['w0'])


@pytest.mark.parametrize('shape', [(33, 70, 9), (1, 512, 1), (130, 40, 1)], ids=lambda s: 'x'.join(map(str, s)))
def test_zero_shift_returns_w0_and_runs_repeat(shape):
    net, w, dd = _single(shape)
    w2, dd2 = net.run()
    assert np.array_equal(w[net.wmask], w2[net.wmask]) and np.array_equal(dd[net.dmask], dd2[net.dmask])
    zero = torch.where(torch.isnan(net.dev['d']), net.dev['d'], torch.zeros_like(net.dev['d']))
    w3, _ = net.run(d=zero)
    assert np.array_equal(w3[net.wmask], net.host['w0'][net.wmask])


def test_five_layer_table_equals_single_layer_calls():
    net = _Net(TABLE, phases=[1, 2, 3, 1, 2])
    assert all(int(net.dev['w0'][o:].data_ptr()) % 16 == 4 * p for o, p in zip(net.woff, [1, 2, 3, 1, 2]))
    w, dd = net.run()
    w2, dd2 = net.run()
    assert np.array_equal(w[net.wmask], w2[net.wmask]) and np.array_equal(dd[net.dmask], dd2[net.dmask])
    for k, shape in enumerate(TABLE):
        one, w1, dd1 = _single(shape)
        assert np.array_equal(net.layer_w(w, k), one.layer_w(w1, 0)), shape
        assert np.array_equal(net.layer_d(dd, k), one.layer_d(dd1, 0)), shape


def test_taps_are_independent():
    shape = (33, 70, 9)
    net, w, dd = _single(shape)
    dat = net.data[0]
    for t in (0, 4, 8):
        d2 = dat['d'].copy()
        d2[t] = -2.0 * d2[t] + 0.5
        dev = net.dev['d'].clone()
        dev[net.doff[0]:net.doff[0] + d2.size] = torch.from_numpy(d2.reshape(-1)).to(DEV)
        w2, _ = net.run(d=dev)
        a, b = net.layer_w(w, 0), net.layer_w(w2, 0)
        others = [x for x in range(9) if x != t]
        assert np.array_equal(a[:, :, others], b[:, :, others]) and not np.array_equal(a[:, :, t], b[:, :, t])
        g2 = dat['g'].copy()
        g2[:, :, others] = g2[:, :, others] * 3.0 + 1.0
        dev = net.dev['g'].clone()
        dev[net.woff[0]:net.woff[0] + g2.size] = torch.from_numpy(g2.reshape(-1)).to(DEV)
        _, dd2 = net.run(g=dev)
        a, b = net.layer_d(dd, 0), net.layer_d(dd2, 0)
        assert np.array_equal(a[t], b[t]) and not np.array_equal(a[others], b[others])


def test_raw_entries_refuse_bad_tensors():
    from rick_amd.svd import apply_tables, grad_tables
    net, _, _ = _single((33, 70, 9))
    v, t = net.dev, net.tables
    w, dd, part = torch.zeros_like(v['w0']), torch.zeros_like(v['d']), torch.zeros(t.npart, device=DEV)
    with pytest.raises(ValueError):
        apply_tables(v['w0'], w.double(), v['u'], v['vt'], v['d'], t)                      # wrong dtype
    with pytest.raises(ValueError):
        apply_tables(v['w0'], w[:-1].clone(), v['u'], v['vt'], v['d'], t)                  # lengths differ
    with pytest.raises(ValueError):
        apply_tables(v['w0'], w, v['u'][::2], v['vt'], v['d'], t)                          # not dense
    with pytest.raises(ValueError):
        apply_tables(v['w0'].cpu(), w, v['u'], v['vt'], v['d'], t)                         # wrong device
    with pytest.raises(ValueError):
        grad_tables(v['g'], v['u'], v['vt'], dd, part[:-1].clone(), t)                     # short partials workspace
    with pytest.raises(ValueError):
        grad_tables(v['g'], v['u'], v['vt'].cpu(), dd, part, t)
    with pytest.raises(ValueError):
        grad_tables(v['g'], v['u'], v['vt'], dd.to(torch.float16), part, t)
    with pytest.raises(RuntimeError):                                                      # the C entry: buffers shorter than the table
        apply_tables(v['w0'][:100].clone(), w[:100].clone(), v['u'], v['vt'], v['d'], t)
    with pytest.raises(RuntimeError):                                                      # the C entry: w == w0
        apply_tables(v['w0'], v['w0'], v['u'], v['vt'], v['d'], t)


# ---- the trainer ---------------------------------------------------------------------------------------------------------------
def _build(size=32):
    from rick_amd.models import Discriminator, Generator
    torch.manual_seed(11)
    g0, d0 = Generator(size, 512, 2), Discriminator(size)

    def make():
        g, d = Generator(size, 512, 2), Discriminator(size)
        g.load_state_dict(g0.state_dict())
        d.load_state_dict(d0.state_dict())
        return g.to(DEV), d.to(DEV)
    return make


@pytest.fixture(scope='module')
def shared_factors():
    """Both trainers start from the same weights: the host decompositions (seconds per 512 x 512 x 9 layer) are computed once."""
    from rick_amd import svd
    memo, real = {}, svd.decompose

    def decompose(w3):
        key = (tuple(w3.shape), w3.detach().cpu().numpy().tobytes())
        if key not in memo:
            memo[key] = real(w3)
        return tuple(x.clone() for x in memo[key])
    svd.decompose = decompose
    yield _build()
    svd.decompose = real


def _trainer(make, **cfg):
    from rick_amd.train import RickTrainer, TrainConfig
    g, d = make()
    g_ema, d_ema = make()
    return RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, **cfg), g, d, g_ema, d_ema)


def _fixed(g):
    gen = torch.Generator(DEV).manual_seed(7)
    g_noise = [torch.randn(n.shape, device=DEV, generator=gen) for n in g.make_noise()]
    return dict(noise=[torch.randn(2, 512, device=DEV, generator=gen)], g_noise=g_noise,
                real=torch.randn(2, 3, 32, 32, device=DEV, generator=gen))


def _capture_at_adam(svd, optim, flat):
    """The masked Adam zeroes the gradient of the frozen elements, so the gradient the adapter's pass read is copied at the top of
    the optimiser step (MaskedFlatAdam.before_step: after the gradient exchange and grads_(), before Adam)."""
    box = {}

    def hook():
        box.update(grad=flat.grad[svd.lo:svd.hi].clone(), dd=svd.fac.grad.clone())
    optim.before_step = hook
    return box


def _rel(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _check_step(svd, box, literal, what):
    """d.grad against the definition on the step's own flat.grad, and the live weights against W0 + U diag(d) Vt for the stepped
    d: every layer against the fp64 torch composition, the layers of `literal` also against svd_f64; bounds as in the parity tests
    (base: the fp32 torch CPU composition on the same inputs)."""
    worst = [0.0, 0.0]
    for n in svd.names:
        co, ci, taps = svd.shape3[n]
        a, b = svd.segment(n)
        i = svd.fac.index[f'd.{n}']
        lo = int(svd.fac.offsets[i])
        U, Vt = svd.u[n].cpu(), svd.vt[n].cpu()
        G = box['grad'][a:b].view(co, ci, taps).cpu()
        d = svd.d[n].detach().cpu()
        got_dd = box['dd'][lo:lo + d.numel()].view(d.shape).cpu()
        got_w, w0 = svd.weight(n).cpu(), svd.snapshot(n).cpu()
        ref_dd = (torch.bmm(U.double().transpose(1, 2), G.double().permute(2, 0, 1)) * Vt.double()).sum(2)
        ref_w = w0.double() + torch.bmm(U.double() * d.double()[:, None, :], Vt.double()).permute(1, 2, 0)
        if n in literal:
            lit_dd, lit_w = svd_f64.grad(G.numpy(), U.numpy(), Vt.numpy()), svd_f64.apply(w0.numpy(), U.numpy(), Vt.numpy(), d.numpy())
            assert np.abs(lit_dd - ref_dd.numpy()).max() <= 1e-12 * np.abs(lit_dd).max() and np.abs(lit_w - ref_w.numpy()).max() <= 1e-12 * np.abs(lit_w).max()
            ref_dd, ref_w = torch.from_numpy(lit_dd), torch.from_numpy(lit_w)
        base_dd = _rel((torch.bmm(U.transpose(1, 2).contiguous(), G.permute(2, 0, 1).contiguous()) * Vt).sum(2), ref_dd)
        base_w = _rel(w0 + torch.bmm(U * d[:, None, :], Vt).permute(1, 2, 0), ref_w)
        e_dd, e_w = _rel(got_dd, ref_dd), _rel(got_w, ref_w)
        assert float(ref_dd.abs().max()) > 0 and bool(d.any()), (what, n)
        assert e_dd <= max(4 * base_dd, FLOOR), (what, n, e_dd, base_dd)
        assert e_w <= max(4 * base_w, FLOOR), (what, n, e_w, base_w)
        worst = [max(worst[0], e_dd / max(4 * base_dd, FLOOR)), max(worst[1], e_w / max(4 * base_w, FLOOR))]
    print(f'svd {what}: device error / bound  dd {worst[0]:.3f}  W^ {worst[1]:.3f}')


def _outside(svd):
    """bool over flat.flat: the elements of the optimised slice that are not adapted."""
    m = torch.zeros(svd.flat.total, dtype=torch.bool, device=DEV)
    m[svd.lo:svd.hi] = True
    return m & ~svd.frozen_mask(rest=True).bool()


def test_g_and_d_step_train_only_singular_values(shared_factors):
    tr = _trainer(shared_factors, svd_adapt=True)
    sg, sd = tr.svd_g, tr.svd_d
    assert [n for n in sg.names if not (n.endswith('.conv.weight') or n.endswith('.conv.modulation.weight'))] == []
    assert len(sg.names) == 2 * sum(1 for n in tr.g_flat.names if n.startswith('convs.') and n.endswith('.conv.weight'))
    assert sd.shape3['final_linear.0.weight'] == (512, 8192, 1) and sd.shape3['final_linear.1.weight'] == (1, 512, 1)
    assert any('.skip.' in n for n in sd.names) and 'final_conv.0.weight' in sd.names and not any(n.startswith('convs.0.') for n in sd.names)
    assert bool((tr.g_optim.mask[sg.lo:sg.hi] == 1).all()) and bool((tr.d_optim.mask[sd.lo:sd.hi] == 1).all())
    fx = _fixed(tr.g)
    with torch.no_grad():
        img0, _ = tr.g(fx['noise'], noise=fx['g_noise'])
        pred0, _ = tr.d(fx['real'])
    g_before, d_before = tr.g_flat.flat.clone(), tr.d_flat.flat.clone()
    box_g, box_d = _capture_at_adam(sg, tr.g_optim, tr.g_flat), _capture_at_adam(sd, tr.d_optim, tr.d_flat)
    tr.g_step(fx['noise'], fx['g_noise'])
    assert torch.equal(tr.d_flat.flat, d_before)
    tr.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'])
    torch.cuda.synchronize()
    assert 'grad' in box_g and 'grad' in box_d
    assert sg.optim.steps == [1] * len(sg.names) and sd.optim.steps == [1] * len(sd.names)
    for svd, flat, before in ((sg, tr.g_flat, g_before), (sd, tr.d_flat, d_before)):
        out = _outside(svd)
        assert bool(out.any()) and torch.equal(flat.flat[out], before[out])                # biases, noise strengths: bit for bit
        assert torch.equal(flat.flat[:svd.lo], before[:svd.lo]) and torch.equal(flat.flat[svd.hi:], before[svd.hi:])
        assert torch.equal(svd.w0, before[svd.lo:svd.hi]) and bool(torch.isfinite(flat.flat).all())
        for n in svd.names:
            assert not torch.equal(svd.weight(n), svd.snapshot(n)), n                      # every adapted layer moved
            assert torch.equal(svd.singular_values(n), svd.s0[n] + svd.d[n].detach())
    _check_step(sg, box_g, {'convs.0.conv.modulation.weight', 'convs.1.conv.weight'}, 'g_step')
    _check_step(sd, box_d, {'final_linear.1.weight', 'convs.1.skip.1.weight'}, 'd_step')
    with torch.no_grad():                                                                  # the packed weights were refreshed
        img1, _ = tr.g(fx['noise'], noise=fx['g_noise'])
        pred1, _ = tr.d(fx['real'])
    assert not torch.equal(img0, img1) and not torch.equal(pred0, pred1)


def test_train_rest_moves_the_other_tensors(shared_factors):
    tr = _trainer(shared_factors, svd_adapt=True, svd_train_rest=True)
    fx = _fixed(tr.g)
    g_before, d_before = tr.g_flat.flat.clone(), tr.d_flat.flat.clone()
    tr.g_step(fx['noise'], fx['g_noise'])
    tr.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'])
    torch.cuda.synchronize()
    for svd, flat, before, optim in ((tr.svd_g, tr.g_flat, g_before, tr.g_optim), (tr.svd_d, tr.d_flat, d_before, tr.d_optim)):
        out = _outside(svd)
        assert not bool(optim.mask[out].any()) and bool(optim.mask[svd.frozen_mask(rest=True).bool()].all())
        moved = flat.flat[out] != before[out]
        assert float(moved.float().mean()) > 0.3                                           # (the padding between tensors stays 0)
        assert any(bool(svd.d[n].any()) for n in svd.names)


def test_graphs_are_refused_and_off_builds_nothing(shared_factors):
    tr = _trainer(shared_factors, svd_adapt=True)
    with pytest.raises(RuntimeError, match='singular-value adaptation'):
        tr.enable_graphs(True)
    with pytest.raises(RuntimeError, match='singular-value adaptation'):
        tr.g_step(None, graph=True)
    with pytest.raises(RuntimeError, match='singular-value adaptation'):
        tr.d_step(torch.zeros(2, 3, 32, 32, device=DEV), None, graph=True)
    off = _trainer(shared_factors)
    assert off.svd_g is None and off.svd_d is None and off.g_optim.mask is None and off.d_optim.mask is None
