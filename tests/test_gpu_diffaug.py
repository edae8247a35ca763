"""DiffAugment's fused HIP kernels (rick_amd/csrc/diffaug.hip) against the fp64 closed form of tests/diffaug_f64.py.

The bound  |err| <= 32 * 2^-24 * max(1, max|x|)  follows from the kernels' pinned arithmetic: out = fma(c s, v, fma(c (1 - s), m, t)),
m = ((v0 + v1) + v2) / 3 in fp32, the mean and t in fp64 with one rounding.  The terms have magnitude at most 3, 1.5, 0.5 and 0.5
times max|x|, about 20 fp32 roundings weighted by those magnitudes; 32 leaves margin (an fp32 emulation of the order on the CPU sat
at 3.3e-7 for |x| <= 1)."""
import functools

import numpy as np
import pytest
import torch

from tests import diffaug_f64 as O

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (5, 9, 9), (3, 12, 20), (2, 32, 32), (2, 256, 256)]
IDS = ['x'.join(map(str, s)) for s in SHAPES]
EPS = 2.0 ** -24
POLICY = 'color,translation,cutout'


def _bound(t):
    return 32 * EPS * max(1.0, float(t.abs().max()))


def _extremes(n, h, w):
    """Pinned extreme records, each repeated for all n images: the largest shifts (+SR, -SC) and their mirror, the cut centre at 0
    and at its maximum, s = 0, s = 2, c = 0.5."""
    from rick_amd.diffaug import cut_bounds, identity_params
    sr, sc = O.shift_range(h), O.shift_range(w)
    rmax, cmax = h - O.cut_size(h) % 2, w - O.cut_size(w) % 2
    out = []
    for b, s, c, tr, tc, orow, ocol in ((0.5, 0.0, 1.5, sr, -sc, 0, 0), (-0.5, 2.0, 0.5, sr, -sc, rmax, cmax),
                                        (0.25, 2.0, 1.5, -sr, sc, 0, cmax)):
        p = identity_params(n)
        p['b'], p['s'], p['c'], p['tr'], p['tc'] = b, s, c, tr, tc
        p['r0'], p['r1'] = cut_bounds(np.full(n, orow), h)
        p['c0'], p['c1'] = cut_bounds(np.full(n, ocol), w)
        out.append(p)
    return out


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs, parameter sets and fp64 references of one shape: computed once, shared by the tests, never modified."""
    from rick_amd.diffaug import draw_params
    n, h, w = shape
    gen = torch.Generator().manual_seed(100 + h * w)
    x = torch.rand(n, 3, h, w, generator=gen) * 2 - 1
    gy = torch.rand(n, 3, h, w, generator=gen) * 2 - 1
    sets = [draw_params(n, h, w, POLICY, generator=gen)] + _extremes(n, h, w)
    refs = [(O.apply(x, p), O.adjoint(gy, p)) for p in sets]
    return x, gy, sets, refs


def _upload(params, h, w):
    from rick_amd.diffaug import check_params, upload_params
    return upload_params(check_params(params, h, w), 'cuda')


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_forward_and_adjoint_match_the_fp64_closed_form(shape):
    from rick_amd.diffaug import DiffAugAdjFn, diffaug_fused
    n, h, w = shape
    x, gy, sets, refs = _case(shape)
    xd, gd = x.cuda(), gy.cuda()
    for k, (p, (want_y, want_g)) in enumerate(zip(sets, refs)):
        blk = _upload(p, h, w)
        ey = float((diffaug_fused(xd, blk).cpu().double() - want_y).abs().max())
        eg = float((DiffAugAdjFn.apply(gd, blk).cpu().double() - want_g).abs().max())
        print(f'diffaug {shape} set {k}: forward err {ey:.3e} (bound {_bound(x):.3e}), adjoint err {eg:.3e} (bound {_bound(gy):.3e})')
        assert ey <= _bound(x), (shape, k, ey)
        assert eg <= _bound(gy), (shape, k, eg)


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_pure_select_is_exact_and_fill_and_cut_are_exact_zeros(shape):
    from rick_amd.diffaug import DiffAugAdjFn, diffaug_fused
    n, h, w = shape
    x, gy, sets, _ = _case(shape)
    xd, gd = x.cuda(), gy.cuda()
    for p in sets:
        # b = 0, s = 1, c = 1: an index-shifted, zero-filled, cut copy, bit for bit, in both directions
        q = p.copy()
        q['b'], q['s'], q['c'] = 0.0, 1.0, 1.0
        blk = _upload(q, h, w)
        assert torch.equal(diffaug_fused(xd, blk).cpu(), O.select(x, q))
        assert torch.equal(DiffAugAdjFn.apply(gd, blk).cpu(), O.select_t(gy, q))
        # any parameters: the fill and the cut are exactly 0.0
        y = diffaug_fused(xd, _upload(p, h, w)).cpu()
        dead = O.select(torch.ones_like(x), p) == 0
        assert bool(dead.any()) and bool((y[dead] == 0).all())


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_closed_family_second_order(shape):
    """grad of |A^T w|^2 w.r.t. w through DiffAugFn -> DiffAugAdjFn -> DiffAugFn(bias=False) == 2 A A^T w of the fp64 oracle (linear
    part only), relative to max|.| within twice the forward bound; the offset shifts only the forward."""
    from rick_amd.diffaug import DiffAugAdjFn, DiffAugFn, diffaug_fused
    n, h, w = shape
    x, gy, sets, _ = _case(shape)
    for k, p in enumerate(sets[:2]):
        blk = _upload(p, h, w)
        xd = x.cuda().requires_grad_(True)
        wd = gy.cuda().requires_grad_(True)
        s = (diffaug_fused(xd, blk) * wd).sum()
        (gx,) = torch.autograd.grad(s, xd, create_graph=True)
        (gw,) = torch.autograd.grad((gx ** 2).sum(), wd)
        want = 2 * O.apply(O.adjoint(gy, p), p, bias=False)
        err = float((gw.cpu().double() - want).abs().max() / want.abs().max())
        print(f'diffaug {shape} set {k}: second-order rel err {err:.3e} (bound {2 * 32 * EPS:.3e})')
        assert err <= 2 * 32 * EPS, (shape, k, err)
        # bias: forward(bias) - forward(no bias) is b on the live elements, nothing elsewhere; the adjoint does not see b
        with torch.no_grad():
            diff = (DiffAugFn.apply(xd, blk, True) - DiffAugFn.apply(xd, blk, False)).cpu().double()
            want_b = O.apply(torch.zeros_like(x), p, bias=True)
            assert float((diff - want_b).abs().max()) <= 2 * _bound(x)
            q = p.copy()
            q['b'] = 0.0
            assert torch.equal(DiffAugAdjFn.apply(wd, blk), DiffAugAdjFn.apply(wd, _upload(q, h, w)))


def test_batch_invariance_and_reproducibility():
    from rick_amd.diffaug import DiffAugAdjFn, diffaug_fused
    for shape in ((5, 9, 9), (5, 32, 32)):
        n, h, w = shape
        from rick_amd.diffaug import draw_params
        gen = torch.Generator().manual_seed(5)
        x = (torch.rand(n, 3, h, w, generator=gen) * 2 - 1).cuda()
        p = draw_params(n, h, w, POLICY, generator=gen)
        blk = _upload(p, h, w)
        y, g = diffaug_fused(x, blk), DiffAugAdjFn.apply(x, blk)
        assert torch.equal(y, diffaug_fused(x, blk)) and torch.equal(g, DiffAugAdjFn.apply(x, blk))
        for k in range(n):
            one = _upload(p[k:k + 1], h, w)
            xk = x[k:k + 1].clone()
            assert torch.equal(diffaug_fused(xk, one)[0], y[k]), (shape, k)
            assert torch.equal(DiffAugAdjFn.apply(xk, one)[0], g[k]), (shape, k)


def test_einval_argument_checks():
    """Argument checks only: every call below returns before anything is launched."""
    from rick_amd._lib import lib, ptr
    from rick_amd.diffaug import PARAM_DTYPE, identity_params
    EINVAL = 22
    n, h, w = 2, 8, 12
    x = torch.zeros(n, 3, h, w, device='cuda')
    y = torch.empty_like(x)
    ws = torch.empty(lib.rick_diffaug_workspace_bytes(n, h, w) // 8, device='cuda', dtype=torch.float64)
    blk = torch.zeros(n * PARAM_DTYPE.itemsize, dtype=torch.uint8, device='cuda')
    good = [ptr(x), ptr(blk), ptr(ws), ptr(y), n, h, w]
    for i in range(4):                                   # null pointers
        a = list(good)
        a[i] = None
        assert lib.rick_diffaug_fwd_f32(*a, 1, None) == EINVAL
        assert lib.rick_diffaug_adj_f32(*a, None) == EINVAL
    for i in (4, 5, 6):                                  # N, H, W below 1
        for v in (0, -1):
            a = list(good)
            a[i] = v
            assert lib.rick_diffaug_fwd_f32(*a, 1, None) == EINVAL
            assert lib.rick_diffaug_adj_f32(*a, None) == EINVAL
    assert lib.rick_diffaug_workspace_bytes(0, h, w) < 0 and lib.rick_diffaug_workspace_bytes(n, 0, w) < 0
    # geometry: checked on the host copy of the block before its upload
    for field, value in (('tr', h), ('tr', -h), ('tc', w), ('tc', -w), ('r0', -1), ('r1', h + 1), ('c0', -1), ('c1', w + 1)):
        p = identity_params(n)
        p[field][n - 1] = value
        assert lib.rick_diffaug_check_params(p.ctypes.data, n, h, w) == EINVAL, (field, value)
    p = identity_params(n)
    assert lib.rick_diffaug_check_params(p.ctypes.data, n, h, w) == 0
    assert lib.rick_diffaug_check_params(None, n, h, w) == EINVAL and lib.rick_diffaug_check_params(p.ctypes.data, 0, h, w) == EINVAL
