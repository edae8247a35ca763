"""CDC's patch-level discriminator and anchor sampling (rick_amd/patchd.py) without a GPU: the composed head against the literal
fp64 restatement of tests/patchd_f64.py, the heads' state, the taps, the early exit of the patch forward (stand-in blocks that count
their calls), the anchor draw, the schedule, the refusals of the C entry points (checked before any HIP call, so the cross-built
library answers them here) and the trainer's validation and schedule.  CPU-only."""
import ctypes

import numpy as np
import pytest
import torch

from rick_amd import patchd
from tests import patchd_f64 as ref

SHAPES = [(1, 4, 1, 1), (2, 8, 3, 5), (3, 36, 7, 9)]


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a.detach().numpy() if torch.is_tensor(a) else a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_composed_head_matches_the_fp64_restatement(shape):
    x, w, b, g, wscale = ref.case(shape)
    x, w, b, g = (t.double() for t in (x, w, b, g))
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    out = patchd.patch_head(x, w, b, wscale)
    assert out.shape == (shape[0], 1, shape[2], shape[3]) and out.dtype == torch.float64
    _close(out, ref.head_fwd(x, w, b, wscale))
    gx, gw, gb = torch.autograd.grad(out, (x, w, b), g)
    rx, rw, rb = ref.head_bwd(x, w, g, out, wscale)
    _close(gx, rx), _close(gw, rw), _close(gb, rb)
    # other slope and gain than the module's defaults
    out2 = patchd.patch_head(x, w, b, wscale, 0.5, 1.25)
    _close(out2, ref.head_fwd(x, w, b, wscale, 0.5, 1.25))


def test_use_kernels_switch_returns_the_previous_setting():
    assert patchd.use_kernels(False) is True
    assert patchd.use_kernels(True) is False
    assert patchd.use_kernels(True) is True


def test_heads_state_dict():
    sd = patchd.PatchHeads().state_dict()
    want = {}
    for i in range(4):
        want[f'new_conv.{i}.0.weight'] = (1, 512, 3, 3)
        want[f'new_conv.{i}.1.bias'] = (1,)
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    small = patchd.PatchHeads(n_heads=2, channels=8)
    assert sorted(small.state_dict()) == ['new_conv.0.0.weight', 'new_conv.0.1.bias', 'new_conv.1.0.weight', 'new_conv.1.1.bias']
    assert small.new_conv[0][0].scale == 1 / (8 * 9) ** 0.5 and not small.new_conv[1][1].bias.any()      # ConvLayer's own init
    x = torch.randn(2, 8, 3, 5, generator=torch.Generator().manual_seed(0))
    conv, act = small.new_conv[1][0], small.new_conv[1][1]
    _close(small(x, 1), ref.head_fwd(x, conv.weight, act.bias, conv.scale), 1e-6)


def test_patch_taps():
    from rick_amd.models import Discriminator
    assert patchd.patch_taps(Discriminator(256)) == [6, 7, 8, 9]
    assert patchd.patch_taps(Discriminator(32)) == [1, 2, 3]
    assert len(patchd.patch_taps(Discriminator(64))) == 4
    assert patchd.patch_taps(Discriminator(256), channels=256) == []          # the 256-channel features are 128 px and 64 px wide


def test_sample_anchor_latents():
    anchors = torch.randn(10, 512, generator=torch.Generator().manual_seed(1))
    for seed, b in ((0, 4), (7, 9)):
        ind = np.random.RandomState(seed).randint(0, 10, size=b)
        z = patchd.sample_anchor_latents(anchors, b, 0.0, rng=np.random.RandomState(seed))
        assert z.shape == (b, 512) and torch.equal(z, anchors[torch.as_tensor(ind)])
        noisy = patchd.sample_anchor_latents(anchors, b, 0.05, rng=np.random.RandomState(seed),
                                             generator=torch.Generator().manual_seed(3))
        again = patchd.sample_anchor_latents(anchors, b, 0.05, rng=np.random.RandomState(seed),
                                             generator=torch.Generator().manual_seed(3))
        assert torch.equal(noisy, again) and not torch.equal(noisy, z)
        expect = anchors[torch.as_tensor(ind)] + 0.05 * torch.randn(b, 512, generator=torch.Generator().manual_seed(3))
        assert torch.equal(noisy, expect)
    np.random.seed(5)                                                          # numpy's global state when no rng is given
    ind = np.random.RandomState(5).randint(0, 10, size=3)
    assert torch.equal(patchd.sample_anchor_latents(anchors, 3, 0.0), anchors[torch.as_tensor(ind)])
    with pytest.raises(ValueError):
        patchd.sample_anchor_latents(anchors[0], 2, 0.1)


def test_draw_patch_schedule():
    rng = np.random.RandomState(0)
    seen = set()
    for i in range(16):
        which, p_ind = patchd.draw_patch(i, 4, 3, rng)
        assert which == i % 4
        assert (p_ind is None) == (which == 0)
        if p_ind is not None:
            assert isinstance(p_ind, int) and 0 <= p_ind < 3
            seen.add(p_ind)
    assert len(seen) > 1
    assert patchd.draw_patch(5, 1, 3, rng) == (0, None)                        # subspace_freq 1: every iteration is an anchor one


class _Counting:
    """Stands in for a module's forward: counts its calls and returns a feature of the right shape that depends on its input."""

    def __init__(self, shape, both=False):
        self.shape, self.both, self.calls = shape, both, 0

    def __call__(self, x, feat=None):
        self.calls += 1
        y = torch.tanh(x.mean()) + torch.arange(float(np.prod(self.shape))).view(self.shape) / np.prod(self.shape)
        if self.both and feat is not None:
            feat += [y + 1.0, y + 2.0]
        return y


def _counted_d():
    from rick_amd.models import Discriminator
    d = Discriminator(32)
    heads = patchd.PatchHeads(n_heads=3, channels=512)
    f = {}
    f['in'] = d.convs[0].forward = _Counting((2, 512, 32, 32))
    for j, hw in ((1, 16), (2, 8), (3, 4)):
        blk = d.convs[j]
        f[f'b{j}'] = blk.forward = _Counting((2, 512, hw, hw), both=True)
        f[f'b{j}.conv1'] = blk.conv1.forward = _Counting((2, 512, 2 * hw, 2 * hw))
        f[f'b{j}.conv2'] = blk.conv2.forward = _Counting((2, 512, hw, hw))
    f['final'] = d.final_conv.forward = _Counting((2, 512, 4, 4))
    return d, heads, f


@pytest.mark.parametrize('p_ind, ran, shape', [(0, {'in': 1, 'b1.conv1': 1}, 32), (1, {'in': 1, 'b1': 1}, 16),
                                                (2, {'in': 1, 'b1': 1, 'b2.conv1': 1}, 16)])
def test_patch_logits_leaves_the_trunk_at_the_tap(p_ind, ran, shape):
    d, heads, f = _counted_d()
    img = torch.zeros(2, 3, 32, 32)
    out = patchd.patch_logits(d, heads, img, p_ind)
    assert out.shape == (2, 1, shape, shape)
    assert {k: c.calls for k, c in f.items() if c.calls} == ran               # a t1 tap: conv1 only; nothing behind the exit block
    # the head of the tap and no other
    conv, act = heads.new_conv[p_ind][0], heads.new_conv[p_ind][1]
    params = [p for h in heads.new_conv for p in h.parameters()]
    grads = torch.autograd.grad(out.sum(), params, allow_unused=True)
    got = [i // 2 for i, g in enumerate(grads) if g is not None]
    assert got == [p_ind, p_ind] and conv.weight.shape == (1, 512, 3, 3) and act.bias.shape == (1,)
    with pytest.raises(ValueError):
        patchd.patch_logits(d, heads, img, 3)


def test_patch_logits_uses_t2_of_the_exit_block():
    d, heads, f = _counted_d()
    img = torch.zeros(2, 3, 32, 32)
    feat = []
    y = f['b1'](f['in'](img), feat)
    f['b1'].calls = f['in'].calls = 0
    conv, act = heads.new_conv[1][0], heads.new_conv[1][1]
    want = patchd.patch_head(feat[1], conv.weight, act.bias, conv.scale, act.negative_slope, act.scale)
    assert torch.equal(patchd.patch_logits(d, heads, img, 1), want) and not torch.equal(feat[1], y)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    from rick_amd._lib import lib
    EINVAL = 22
    buf = (ctypes.c_float * 4096)()
    base = (ctypes.addressof(buf) + 63) // 64 * 64                            # host memory: every call below must return before a launch
    x, w, b, out, g, gx, ws = (base + 1024 * k for k in range(7))
    cfg = (1.0, 0.2, 1.4, None)
    fwd = lambda *a: lib.rick_patch_head_fwd_f32(*a, *cfg)                    # noqa: E731
    bwd = lambda *a: lib.rick_patch_head_bwd_f32(*a, *cfg)                    # noqa: E731
    fin = lambda *a: lib.rick_patch_head_bwd_finish_f32(*a, 1.0, None)        # noqa: E731
    for C in (6, 2, 0, 2052, 4096):                                           # C % 4 != 0, C < 4, C > 2048
        assert fwd(x, w, b, out, 1, 2, 2, C) == EINVAL
        assert bwd(x, w, g, out, gx, ws, 1, 2, 2, C) == EINVAL
        assert fin(ws, gx, b, 1, 2, 2, C) == EINVAL
        assert lib.rick_patch_head_workspace_bytes(1, 2, 2, C) == -1
    for dims in ((0, 2, 2, 8), (1, 0, 2, 8), (1, 2, 0, 8), (4, 1024, 1024, 512)):     # an empty dimension; 2^31 elements
        assert fwd(x, w, b, out, *dims) == EINVAL and bwd(x, w, g, out, gx, ws, *dims) == EINVAL
        assert lib.rick_patch_head_workspace_bytes(*dims) == -1
    ok = (x, w, b, out)
    for k in range(4):                                                        # a NULL operand
        args = list(ok)
        args[k] = None
        assert fwd(*args, 1, 2, 2, 8) == EINVAL
    ok = (x, w, g, out, gx, ws)
    for k in (0, 1, 2, 3, 5):                                                 # (gx may be NULL)
        args = list(ok)
        args[k] = None
        assert bwd(*args, 1, 2, 2, 8) == EINVAL
    for args in ((None, gx, b), (ws, None, b), (ws, gx, None)):
        assert fin(*args, 1, 2, 2, 8) == EINVAL
    assert fwd(x + 4, w, b, out, 1, 2, 2, 8) == EINVAL                        # 16-byte alignment of x and w
    assert fwd(x, w + 8, b, out, 1, 2, 2, 8) == EINVAL
    assert fwd(x, w, b + 2, out, 1, 2, 2, 8) == EINVAL                        # 4-byte alignment of the rest
    assert bwd(x, w, g, out, gx + 4, ws, 1, 2, 2, 8) == EINVAL
    assert bwd(x, w, g + 1, out, gx, ws, 1, 2, 2, 8) == EINVAL
    assert bwd(x, w, g, out, x, ws, 1, 2, 2, 8) == EINVAL                     # gx == x
    assert fin(ws + 4, gx, b, 1, 2, 2, 8) == EINVAL                           # ws holds doubles: 8-byte alignment
    assert bwd(x, w, g, out, gx, ws + 4, 1, 2, 2, 8) == EINVAL
    # the partition is a function of the sizes alone: slabs of 32 pixels up to 512 slabs, then longer slabs
    assert lib.rick_patch_head_workspace_bytes(4, 32, 32, 512) == 128 * (9 * 512 * 4 + 8)
    assert lib.rick_patch_head_workspace_bytes(1, 1, 1, 4) == 9 * 4 * 4 + 8
    assert lib.rick_patch_head_workspace_bytes(1, 129, 128, 4) == 258 * (9 * 4 * 4 + 8)


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


def _make(dp=None, patch_heads=None, sources=False, **cfg):
    from rick_amd.train import RickTrainer, TrainConfig
    build = _build()
    g, d = build()
    g_ema, d_ema = build()
    gs, ds = build() if sources else (None, None)
    return RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, **cfg), g, d, g_ema, d_ema, dp=dp, g_source=gs,
                       d_source=ds, patch_heads=patch_heads)


def test_config_defaults_are_off():
    from rick_amd.train import TrainConfig
    c = TrainConfig()
    assert (c.subspace_freq, c.subspace_std, c.feat_ind, c.n_anchors) == (0, 0.05, 3, 10)
    tr = _make()
    assert tr.patch_heads is None and tr.anchors is None and tr.head_flat is None and tr.head_optim is None
    with pytest.raises(ValueError, match='subspace_freq'):
        tr.d_step(torch.zeros(2, 3, 32, 32), None, patch=0)
    with pytest.raises(ValueError, match='subspace_freq'):
        tr.g_step(None, patch=0)


def test_trainer_validation():
    class _Dp:
        world = 1

        def attach(self, *flats):
            pass
    with pytest.raises(ValueError, match='not built'):
        _make(dp=_Dp(), subspace_freq=4)
    with pytest.raises(ValueError, match='not built'):
        _make(sources=True, subspace_freq=4, dcl_d_weight=0.5)
    with pytest.raises(ValueError, match='feat_ind'):
        _make(subspace_freq=4, feat_ind=4)                                     # a 32-px discriminator has three taps
    with pytest.raises(ValueError, match='feat_ind'):
        _make(subspace_freq=4, feat_ind=0)
    with pytest.raises(ValueError, match='feat_ind'):
        _make(subspace_freq=4, feat_ind=3, patch_heads=patchd.PatchHeads(n_heads=2))
    for bad in (dict(subspace_freq=-1), dict(subspace_freq=2.0), dict(subspace_freq=True)):
        with pytest.raises(ValueError, match='subspace_freq'):
            _make(**bad)
    for bad in (dict(n_anchors=0), dict(subspace_std=-0.1), dict(subspace_std=float('nan'))):
        with pytest.raises(ValueError, match='n_anchors'):
            _make(subspace_freq=4, **bad)
    with pytest.raises(ValueError, match='patch_heads'):
        _make(patch_heads=patchd.PatchHeads())
    _make(sources=True, subspace_freq=4, dcl_g_weight=2.0, cdc_weight=1000.0)   # the generator-side terms go with it
    heads = patchd.PatchHeads(n_heads=3)
    tr = _make(subspace_freq=4, patch_heads=heads, n_anchors=6)
    assert tr.patch_heads is heads and tr.anchors.shape == (6, 512) and tr.last_patch is None
    # the heads live in a flat buffer of their own with an Adam at D's learning rate and betas
    assert tr.head_flat.params == list(heads.parameters()) and tr.head_optim.lr == tr.d_optim.lr
    assert tuple(tr.head_optim.betas) == tuple(tr.d_optim.betas) and tr.head_optim.mask is None
    assert all(p.data_ptr() == tr.head_flat.flat[o:].data_ptr() for p, o in zip(heads.parameters(), tr.head_flat.offsets))
    built = _make(subspace_freq=4)
    assert isinstance(built.patch_heads, patchd.PatchHeads) and len(built.patch_heads.new_conv) == 4


def test_iteration_follows_the_schedule():
    """Stand-ins for the step methods record what `iteration` hands them: anchor iterations pass one anchor-subspace latent batch
    to both steps and no tap; the others pass the same drawn tap to both and ordinary mixing noise."""
    tr = _make(subspace_freq=4, subspace_std=0.0, d_reg_every=4, g_reg_every=4)
    log = []
    tr.d_step = lambda real, noise, i, graph=False, **kw: log.append(('d', noise, kw))
    tr.g_step = lambda noise, graph=False, **kw: log.append(('g', noise, kw))
    tr.r1_step = lambda real, i, graph=False: log.append(('r1', None, {}))
    tr.plr_step = lambda noise, graph=False: log.append(('plr', noise, {}))
    tr.ema_step = lambda: log.append(('ema', None, {}))
    real = torch.zeros(2, 3, 32, 32)
    np.random.seed(3)
    taps = set()
    for i in range(8):
        del log[:]
        tr.iteration(i, real)
        names = [n for n, _, _ in log]
        assert names == (['d', 'r1', 'g', 'plr', 'ema'] if i % 4 == 0 else ['d', 'g', 'ema'])
        (_, dz, dkw), (_, gz, gkw) = [e for e in log if e[0] in 'dg']
        which, p_ind = tr.last_patch
        assert which == i % 4
        if which == 0:
            assert p_ind is None and dkw == {} and gkw == {}
            for z in (dz, gz):                                                 # std = 0: rows of the anchor matrix, exactly
                assert len(z) == 1 and z[0].shape == (2, 512)
                assert all(any(torch.equal(r, a) for a in tr.anchors) for r in z[0])
        else:
            assert dkw == {'patch': p_ind} and gkw == {'patch': p_ind} and 0 <= p_ind < 3
            assert len(dz) in (1, 2) and dz[0].shape == (2, 512)              # mixing noise, as without the feature
            taps.add(p_ind)
    assert len(taps) > 1
    tr.anchors = torch.ones(1, 512)                                            # the anchors can be set
    del log[:]
    tr.iteration(8, real)
    assert torch.equal(log[0][1][0], torch.ones(2, 512))
    off = _make()
    del log[:]
    off.d_step = lambda real, noise, i, graph=False, **kw: log.append(('d', noise, kw))
    off.g_step = lambda noise, graph=False, **kw: log.append(('g', noise, kw))
    off.r1_step = off.plr_step = lambda *a, **k: None
    off.ema_step = lambda: None
    off.iteration(1, real)
    assert [(n, kw) for n, _, kw in log] == [('d', {}), ('g', {})] and off.last_patch is None
