"""The four ADA augmentation kernels (aug_warp_fwd_kernel, aug_down_fwd_kernel, aug_down_adj_kernel, aug_warp_adj_kernel,
rick_amd/csrc/augment.hip) through the C ABI (rick_augment_fwd_f32, rick_augment_adj_f32, rick_augment_workspace_floats) on raw
pointers, per element against the fp64 restatement of include/rick_hip.h's rick_aug_param semantics in tests/ada_f64.py (index
gathers and two plain convolutions; random_apply_affine, upfirdn2d and grid_sample are not used; the adjoint reference is fp64
autograd of <out, gy>, the exact transpose).

Cases are small and mostly not square: a given G, a random colour matrix, (H, W) and the pads draw_affine gives.  Every case
states as literals the edge geometries it reaches (FEATURES); the host-only test recomputes them from the parameter block and
the reference's structure (ada_f64.features), holds the literals to that, and asserts that every feature is reached.  Every case
runs forward AND adjoint, so a feature that concerns both is reached by both.  mirror-lo / mirror-hi: a reflected copy of a
source pixel carries weight to some output; -edge: the outermost canvas row / column does, i.e. the copy of the last source
pixel that has one (s == lo + 6, resp. s == n - 1 - (hi + 6); s == lo + 7 has none: its copy would lie outside the canvas).
pad-limit asks for a pad > 0 with pad + 6 == n - 1 (the 7-pixel images meet the equation with pad 0: min-image).

Checks.

  bound  per element, forward (with the colour offset) and adjoint, uniform random images in [-1, 1) and single-pixel deltas
         (forward x = e_s without the offset, adjoint gy = e_t; every border pixel and three interior ones of the DELTA cases,
         one launch of as many samples under the one entry):
             |dev - ref64| <= (K + R) * 2**-24 * S_tight + R_w * 2**-24 * S_corner
         S_tight: the pipeline on |x| with |k2|, |col| and the exact weights; S_corner: the same with every in-canvas corner weight
         replaced by 1.  No term relative to ref: where both are 0 (no path reaches the element; every delta case beyond 7 x 7 has
         such elements, asserted on the host) the result must be an exact 0.
         K, the fma chains an element's terms pass through.  Forward 36 + 4 + 144 + 3: the polyphase taps of up_value, the four
         corners, the down FIR, the colour row (the offset is the chain's start: no rounding).  Adjoint 36 + 3 + 4 + chain:
         aug_down_adj_kernel's taps (at most 6 x 6), its colour column (one product and two fmas), the corners summed into wsum,
         and `chain`, the (reflect copy, region pixel) pairs aug_warp_adj_kernel accumulates for that source pixel, counted per
         element from the reference's structure (ada_f64.adj_chain: the pairs with a corner inside the copy's clipped tap box,
         which is exactly the kernel's `continue` test).  Every fma rounds once and k2(a, b) is the reference's own fp32 product,
         so no further rounding carries a relative error: R = 1 stands for the second-order terms ((1 + u)**K <= 1 + (K + 1) u
         for K**2 u < 2; K stays below 2000 here).
         R_w = 5, the roundings of a bilinear weight, each an absolute error of at most 2**-24 on a weight <= 1 (2**-25 in
         fact, which leaves room for their products): (float)(ix - floor) on either axis (2; ix, iy themselves are the
         reference's, bit for bit: two fp64 fmas each, emulated exactly), 1 - f on either axis (2), wy * wx (1).  They have no
         bound relative to the weight (1 - fx when fx rounds to 1), hence S_corner.  Nothing is measured.
  sharp  max |dev - ref64| / max |ref64| <= FACTOR * base, FACTOR = 4, base the same figure of an fp32 CPU evaluation of the
         definition in the kernels' order (ada_f64.apply_f32 / adjoint_f32: tap by tap, vectorised over pixels) against the fp64
         reference, on the random data of the case; measured on the CPU against the reference, never against the kernel, and
         recorded in CPU_BASE (regenerate: python -c "from tests.test_gpu_ada_forms import cpu_bases as f; f()").
  exact  (torch.equal) a sample alone gives the bits it has in the mixed-pad batch of its (H, W) (one launch over the entries of
         different cases, as the D step's cat(fake, real)), forward and adjoint; two launches agree; with col[:, :3] = I and a
         zero offset bias = 0 equals bias = 1; a permutation colour matrix gives the identity-colour output with its channels
         permuted, forward and adjoint (row-major col and its transpose); col[:, :3] = 0 with bias = 1 gives col[:, 3]
         everywhere; bias = 0 ignores the offset.
  guard  out, gx and the workspace (exactly rick_augment_workspace_floats floats, = N * 3 * (2H + 10) * (2W + 10)) lie between
         sentinel bands that stay intact; x and gy are views into NaN-fenced buffers; the parameter block is a view into a byte
         buffer whose neighbouring entries hold NaN matrices and huge pads; no output is ever NaN.
  refusals  each null pointer, N < 1, H or W = 6, H or W > 16384: status 22, outputs and workspace untouched.

Host-only (no GPU): ada_f64 against apply_color(random_apply_affine(...)) in fp64 on every case, its autograd adjoint against the composed
path's autograd, and against the recorded outputs auga / augb / augc of the `ada` fixture, all within the tolerance
tests/test_augment_fused.py uses for the same comparison, 2e-5 * max(1, size / 32) * max(1, |ref|) (the residue is the composed
path's fp32 linspace); the feature replay; and the checks themselves, held to planted faults: the fp32 CPU evaluation of the
adjoint with the outermost reflect copy dropped, with a tap box one region pixel short, or with the colour matrix transposed
must miss the bound the device is held to, and pass it when honest.

Features no small geometry reaches: none."""
import functools
import math
import types

import numpy as np
import pytest
import torch

from tests import ada_f64 as A
from tests.forms_common import DEV, SENT, Fenced, Guarded, _gen, fenced, p, stream

gpu = pytest.mark.gpu
EINVAL = 22
U = 2.0 ** -24
K_FWD = 36 + 4 + 144 + 3
K_ADJ = 36 + 3 + 4            # + the per-element chain of aug_warp_adj_kernel
R, R_W = 1, 5                 # module docstring
FACTOR = 4
FEATURES = {'pad0', 'pad-asym', 'pad-xy-differ', 'pad-limit', 'min-image', 'min-image-7xW', 'oob-corner', 'int-coords', 'flip',
            'rot90-nonsquare', 'rotation', 'aniso', 'mirror-lo', 'mirror-hi', 'mirror-lo-edge', 'mirror-hi-edge'}


def _rot(t):
    c, s = math.cos(t), math.sin(t)
    return torch.tensor([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def _sc(sx, sy):
    return torch.tensor([[sx, 0, 0], [0, sy, 0], [0, 0, 1.0]])


def _tr(tx, ty):
    return torch.tensor([[1, 0, tx], [0, 1, ty], [0, 0, 1.0]])


def case(cid, H, W, G, pads, feat, deltas=False):
    return types.SimpleNamespace(id=cid, H=H, W=W, G=G, pads=pads, feat=set(feat.split()), deltas=deltas)


EYE, QUARTER = torch.eye(3), _rot(-math.pi / 2)
CASES = [
    case('id-7x7', 7, 7, EYE, (0, 0, 0, 0), 'min-image mirror-hi mirror-lo mirror-lo-edge oob-corner pad0', deltas=True),
    case('rot90-7x7', 7, 7, QUARTER, (0, 0, 0, 0), 'int-coords min-image mirror-hi mirror-lo mirror-lo-edge oob-corner pad0', deltas=True),
    case('id-7x9', 7, 9, EYE, (0, 0, 0, 0), 'min-image-7xW mirror-hi mirror-lo mirror-lo-edge oob-corner pad0', deltas=True),
    case('flip-zoomout-7x9', 7, 9, _sc(-0.85, 1), (2, 2, 0, 0),
         'aniso flip min-image-7xW mirror-hi mirror-lo mirror-lo-edge oob-corner pad-limit pad-xy-differ pad0', deltas=True),
    case('id-9x13', 9, 13, EYE, (0, 0, 0, 0), 'int-coords mirror-hi mirror-lo mirror-lo-edge oob-corner pad0', deltas=True),
    case('rot180-zoomout-9x13', 9, 13, _sc(-0.9, -0.9), (2, 2, 2, 1), 'mirror-hi mirror-lo pad-limit'),
    case('id-12x7', 12, 7, EYE, (0, 0, 0, 0), 'int-coords mirror-hi mirror-lo mirror-lo-edge oob-corner pad0'),
    case('rot90-12x7', 12, 7, QUARTER, (0, 0, 0, 0),
         'mirror-hi mirror-hi-edge mirror-lo mirror-lo-edge oob-corner pad0 rot90-nonsquare', deltas=True),
    case('rot90-12x12', 12, 12, QUARTER, (0, 0, 0, 0), 'int-coords mirror-hi mirror-lo mirror-lo-edge oob-corner pad0'),
    case('aniso-12x12', 12, 12, _sc(0.9, 1.2), (2, 2, 0, 0), 'aniso mirror-hi mirror-lo pad0'),
    case('rot90-16x24', 16, 24, QUARTER, (0, 0, 0, 0),
         'int-coords mirror-hi mirror-hi-edge mirror-lo mirror-lo-edge oob-corner pad0 rot90-nonsquare'),
    case('zoom-shift-16x24', 16, 24, torch.tensor([[1.1, 0, 0.2], [0, 1.1, 0.1], [0, 0, 1.0]]), (3, 0, 0, 0),
         'mirror-hi mirror-lo mirror-lo-edge oob-corner pad-xy-differ pad0'),
    case('aniso-11x16', 11, 16, _sc(1.15, 0.9), (0, 0, 2, 2), 'aniso mirror-hi mirror-lo pad-xy-differ pad0'),
    case('limit-11x16', 11, 16, torch.tensor([[0.74, 0, 0.1], [0, 0.74, 0], [0, 0, 1.0]]), (8, 4, 4, 4),
         'mirror-hi mirror-lo pad-limit pad-xy-differ', deltas=True),
    case('rot-16x12', 16, 12, _rot(0.3), (4, 4, 5, 5), 'mirror-hi mirror-lo pad-xy-differ rotation'),
    case('zoomout-16x12', 16, 12, _sc(0.8, 0.8), (3, 3, 4, 4), 'mirror-hi mirror-lo pad-xy-differ'),
    case('rot-20x14', 20, 14, _rot(-0.2) @ _tr(0.05, -0.03), (4, 2, 3, 5), 'mirror-hi mirror-lo pad-asym pad-xy-differ rotation'),
    case('fliprot-20x14', 20, 14, _sc(-1, 1) @ _rot(0.25), (4, 4, 5, 5), 'flip mirror-hi mirror-lo pad-xy-differ rotation'),
    case('limit-24x17', 24, 17, torch.tensor([[0.7, 0, 0.1], [0, 0.7, 0], [0, 0, 1.0]]), (10, 5, 11, 11),
         'mirror-hi mirror-lo pad-limit pad-xy-differ'),
    case('shift-24x17', 24, 17, _tr(0.3, 0.0), (6, 0, 0, 0), 'int-coords mirror-hi mirror-lo mirror-lo-edge oob-corner pad-xy-differ pad0'),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
SHAPES = sorted({(c.H, c.W) for c in CASES})
# max |fp32 CPU evaluation in the kernels' order - ref64| / max |ref64| on case_data(id): (forward, adjoint)
CPU_BASE = {
    'id-7x7': (4.415e-07, 7.715e-07),
    'rot90-7x7': (3.609e-07, 1.140e-06),
    'id-7x9': (2.427e-07, 7.189e-07),
    'flip-zoomout-7x9': (1.451e-07, 9.342e-07),
    'id-9x13': (1.756e-07, 8.413e-07),
    'rot180-zoomout-9x13': (2.879e-07, 9.696e-07),
    'id-12x7': (2.129e-07, 6.885e-07),
    'rot90-12x7': (2.069e-07, 8.316e-07),
    'rot90-12x12': (3.748e-07, 4.280e-07),
    'aniso-12x12': (2.351e-07, 6.701e-07),
    'rot90-16x24': (3.042e-07, 1.243e-06),
    'zoom-shift-16x24': (3.151e-07, 5.934e-07),
    'aniso-11x16': (3.856e-07, 6.373e-07),
    'limit-11x16': (3.156e-07, 5.014e-07),
    'rot-16x12': (2.195e-07, 6.583e-07),
    'zoomout-16x12': (1.878e-07, 6.152e-07),
    'rot-20x14': (2.821e-07, 6.548e-07),
    'fliprot-20x14': (1.822e-07, 3.686e-07),
    'limit-24x17': (3.015e-07, 4.784e-07),
    'shift-24x17': (2.762e-07, 5.643e-07),
}


# -------------------------------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def case_data(cid):
    """Block entry, operands and every fp64 figure of a case, computed once and left unchanged."""
    from rick_amd.augment import aug_params, draw_affine
    c = BY_ID[cid]
    g = _gen('ada/' + cid)
    G = c.G[None].float()
    _, pads = draw_affine(1.0, 1, c.H, c.W, G)
    C = torch.randn(1, 4, 4, generator=g) * 0.5 + torch.eye(4)
    d = types.SimpleNamespace(G=G, C=C, pads=pads, blk=aug_params(G, C, c.H, c.W, pads))
    d.s = A.structure(d.blk[0], c.H, c.W)
    d.x = torch.rand(3, c.H, c.W, generator=g) * 2 - 1
    d.gy = torch.rand(3, c.H, c.W, generator=g) * 2 - 1
    d.chain = A.adj_chain(d.blk[0], c.H, c.W, d.s)
    d.fwd = figures(d, d.x, 'fwd', True)
    d.adj = figures(d, d.gy, 'adj')
    return d


def figures(d, v, kind, bias=False):
    """(ref64, bound) of the forward of x = v or of the adjoint of gy = v ([3, H, W] or [B, 3, H, W])."""
    if kind == 'fwd':
        ref, st, sc = (A.apply(v, d.blk[0], bias, mode, d.s) for mode in ('value', 'tight', 'corner'))
        K = K_FWD
    else:
        ref, st, sc = (A.adjoint(v, d.blk[0], mode, d.s) for mode in ('value', 'tight', 'corner'))
        K = K_ADJ + d.chain
    assert bool((sc >= st * (1 - 1e-12)).all())
    return ref, (K + R) * U * st + R_W * U * sc


def delta_inputs(c):
    """[B, 3, H, W]: one 1 per image, at every border pixel and three interior ones, the channel cycling."""
    pix = [(i, j) for i in range(c.H) for j in range(c.W) if i in (0, c.H - 1) or j in (0, c.W - 1)]
    pix += [(1, 1), (c.H // 2, c.W // 2), (c.H - 2, c.W - 3)]
    v = torch.zeros(len(pix), 3, c.H, c.W)
    for k, (i, j) in enumerate(pix):
        v[k, k % 3, i, j] = 1
    return v


@functools.lru_cache(maxsize=None)
def delta_data(cid):
    c, d = BY_ID[cid], case_data(cid)
    v = delta_inputs(c)
    return v, figures(d, v, 'fwd'), figures(d, v, 'adj')


def max_rel_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def cpu_bases():
    """Prints CPU_BASE: the fp32 CPU evaluation in the kernels' order against the fp64 reference, on the CPU alone."""
    for c in CASES:
        d = case_data(c.id)
        print(f"    '{c.id}': ({max_rel_err(A.apply_f32(d.x, d.blk[0]), d.fwd[0]):.3e}, "
              f"{max_rel_err(A.adjoint_f32(d.gy, d.blk[0]), d.adj[0]):.3e}),")


def print_features():
    for c in CASES:
        d = case_data(c.id)
        print(f"{c.id}: {d.pads} '{' '.join(sorted(A.features(d.blk[0], c.H, c.W, d.s)))}'")


# ------------------------------------------------------------------------------------------------------ host-only tests
def tolerance(c, ref):
    return 2e-5 * max(1.0, max(c.H, c.W) / 32) * max(1.0, float(ref.abs().max()))


def test_feature_literals_replay_and_coverage():
    reached = set()
    for c in CASES:
        d = case_data(c.id)
        assert d.pads == c.pads, (c.id, d.pads)
        assert A.pads_of(d.blk[0], c.H, c.W) == c.pads
        got = A.features(d.blk[0], c.H, c.W, d.s)
        assert got == c.feat, (c.id, sorted(got ^ c.feat))
        assert c.H <= 24 and c.W <= 24
        assert int(d.chain.min()) >= 1 and float(d.fwd[1].min()) > 0
        reached |= got
    assert reached == FEATURES, sorted(FEATURES - reached)
    # the deltas see the mirrored copies and the canvas edge where a missing path shows
    delta_feat = set().union(*(c.feat for c in CASES if c.deltas))
    assert {'mirror-lo', 'mirror-hi', 'mirror-lo-edge', 'mirror-hi-edge', 'oob-corner', 'int-coords', 'pad-limit', 'flip'} <= delta_feat
    assert set(CPU_BASE) == set(BY_ID)
    # but on the 7 x 7 images, where the 12 taps span everything, some delta never reaches some element: an exact 0 is required
    for c in CASES:
        if c.deltas:
            d, (v, fwd, adj) = case_data(c.id), delta_data(c.id)
            assert all(bool((bound == 0).any()) == (c.H * c.W > 49) for _, bound in (fwd, adj)), c.id
            # and the bound is 0 exactly where the indicator pipeline counts no path
            assert torch.equal(fwd[1] == 0, A.apply(v, d.blk[0], False, 'count', d.s) == 0), c.id
            assert torch.equal(adj[1] == 0, A.adjoint(v, d.blk[0], 'count', d.s) == 0), c.id
    for hw in SHAPES:                                                     # the mixed-pad launches do mix
        assert len([c for c in CASES if (c.H, c.W) == hw]) >= 2


def test_chain_count_against_the_indicator_pipeline():
    """adj_chain counts (copy, region pixel) pairs; the transposed indicator pipeline of the warp alone counts (copy, tap,
    corner) paths: between 1 and 4 per pair."""
    for cid in ('id-7x7', 'limit-11x16', 'fliprot-20x14'):
        c, d = BY_ID[cid], case_data(cid)
        padded = torch.zeros(3, d.s['hp'], d.s['wp'], dtype=torch.float64, requires_grad=True)
        k2 = torch.ones(12, 12, dtype=torch.float64)
        z = torch.zeros(3, 2 * d.s['hp'], 2 * d.s['wp'], dtype=torch.float64)
        z[:, ::2, ::2] = padded
        up = torch.nn.functional.conv2d(z[:, None], k2[None, None])[:, 0].reshape(3, -1)
        paths = sum((up[:, idx] * inside.reshape(-1)).sum() for idx, _, inside in A.corners(d.s))
        per_canvas = torch.autograd.grad(paths, padded)[0][0]
        per_source = torch.zeros(c.H, c.W, dtype=torch.float64)
        per_source.index_put_((torch.from_numpy(d.s['ri'])[:, None].expand(-1, d.s['wp']),
                               torch.from_numpy(d.s['ci'])[None, :].expand(d.s['hp'], -1)), per_canvas, accumulate=True)
        assert bool((d.chain <= per_source).all()) and bool((per_source <= 4 * d.chain).all()), cid


def beyond(got, fig):
    return int(((got.double() - fig[0]).abs() > fig[1]).sum())


@pytest.mark.parametrize('fault', ['edge-copy', 'short-box', 'colour'])
def test_the_checks_notice_a_planted_fault(fault):
    """The fp32 evaluation of the adjoint with an index fault planted (ada_f64.adjoint_f32) against the checks the device gets:
    honest, it passes the bound and FACTOR x its own base; with a dropped edge copy or a tap box one pixel short the delta
    bound fails, with a transposed colour matrix the random-data bound does."""
    cid = 'id-7x9'
    d = case_data(cid)
    v, _, adj = delta_data(cid)
    run = lambda g, f: torch.stack([A.adjoint_f32(gk, d.blk[0], f) for gk in g.reshape(-1, 3, 7, 9)])
    some = slice(0, 6)                                                    # deltas along the first row: the low mirrored copies
    honest, faulty = run(v[some], None), run(v[some], fault)
    assert beyond(honest, (adj[0][some], adj[1][some])) == 0 and beyond(run(d.gy, None)[0], d.adj) == 0
    caught = beyond(faulty, (adj[0][some], adj[1][some])) + beyond(run(d.gy, fault)[0], d.adj)
    print(f'{fault}: {caught} elements beyond the bound')
    assert caught > 0
    if fault != 'colour':
        assert beyond(faulty, (adj[0][some], adj[1][some])) > 0


@pytest.mark.parametrize('cid', list(BY_ID))
def test_reference_against_the_composed_path(cid):
    from rick_amd.augment import apply_color, random_apply_affine
    c, d = BY_ID[cid], case_data(cid)
    x = d.x.double()[None].requires_grad_(True)
    ref = apply_color(random_apply_affine(x, 1.0, d.G)[0], d.C)
    err = float((d.fwd[0] - ref[0].detach()).abs().max())
    (gref,) = torch.autograd.grad((ref[0] * d.gy.double()).sum(), x)
    gerr = float((d.adj[0] - gref[0]).abs().max())
    print(f'{cid}: forward {err:.2e} (|ref| {float(ref.detach().abs().max()):.2f}), adjoint {gerr:.2e} (|ref| {float(gref.abs().max()):.2f})')
    assert err < tolerance(c, ref.detach()) and gerr < tolerance(c, gref)
    # the fp32 evaluations the CPU bases come from are evaluations of the same definition
    if c.H * c.W <= 63:
        assert max_rel_err(A.apply_f32(d.x, d.blk[0]), d.fwd[0]) < 1e-5
        assert max_rel_err(A.adjoint_f32(d.gy, d.blk[0]), d.adj[0]) < 1e-5


@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_reference_against_the_recorded_fixtures(golden, tag):
    from rick_amd.augment import _padding, aug_params
    g = golden('ada')
    img, ref = torch.from_numpy(g[f'aug{tag}/img']), torch.from_numpy(g[f'aug{tag}/out']).double()
    G, C = torch.from_numpy(g[f'aug{tag}/G']), torch.from_numpy(g[f'aug{tag}/C'])
    h, w = img.shape[2:]
    blk = aug_params(G, C, h, w, _padding(torch.inverse(G.float()), h, w))
    out = torch.stack([A.apply(img[n], blk[n]) for n in range(img.shape[0])])
    tol = 2e-5 * max(1.0, max(h, w) / 32) * max(1.0, float(ref.abs().max()))
    assert float((out - ref).abs().max()) < tol


# ---------------------------------------------------------------------------------------------------------- launches
def param_buffer(blk):
    """The entries between two poisoned neighbours (NaN matrices, huge pads) in one byte buffer -> (buffer, pointer)."""
    from rick_amd.augment import PARAM_DTYPE
    full = np.zeros(blk.shape[0] + 2, PARAM_DTYPE)
    full[1:-1] = blk
    for k in (0, -1):
        full['a'][k], full['ainv'][k], full['col'][k] = np.nan, np.nan, np.nan
        full['py1'][k] = full['px1'][k] = 1 << 20
        full['hp'][k] = full['wp'][k] = 1 << 24
    buf = torch.from_numpy(full.view(np.uint8).copy()).to(DEV)
    assert buf.numel() == (blk.shape[0] + 2) * 144 and buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 144


def launch(kind, blk, v, bias=1):
    """One call on a fenced operand, the poisoned parameter buffer, a guarded workspace and a guarded output -> [N, 3, H, W]."""
    from rick_amd._lib import lib
    v = v.float().reshape(-1, 3, v.shape[-2], v.shape[-1])
    N, _, H, W = v.shape
    assert blk.shape == (N,)
    nws = lib.rick_augment_workspace_floats(N, H, W)
    assert nws == N * 3 * (2 * H + 10) * (2 * W + 10)
    src, ws, dst = fenced(v), Guarded(nws), Guarded(v.numel())
    buf, prm = param_buffer(blk)
    if kind == 'fwd':
        rc = lib.rick_augment_fwd_f32(p(src), prm, p(ws), p(dst), N, H, W, bias, stream())
    else:
        rc = lib.rick_augment_adj_f32(p(src), prm, p(ws), p(dst), N, H, W, stream())
    assert rc == 0, f'{kind}: status {rc}'
    torch.cuda.synchronize()
    ws.assert_bands(f'{kind} workspace')
    dst.assert_bands(f'{kind} output')
    out = dst.v.cpu().view(N, 3, H, W)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(ws.v).all()), f'{kind}: non-finite output or workspace'
    assert not bool((out == SENT).any()), f'{kind}: an output element was not written'
    return out


def hold_to_bound(what, got, ref, bound):
    err = (got.double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f'{what} bound: max |d| {float(err.max()):.3e}, worst |d| / bound {float(ratio.reshape(-1)[i]):.3f} '
          f'(|d| {float(err.reshape(-1)[i]):.3e} against {float(bound.reshape(-1)[i]):.3e}), exact zeros {int((bound == 0).sum())}')
    bad = err > bound
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} elements beyond the bound, first at {bad.nonzero()[0].tolist()}'


@gpu
@pytest.mark.parametrize('cid', list(BY_ID))
def test_case_bound_and_sharp(cid):
    d = case_data(cid)
    for k, (kind, v, (ref, bound)) in enumerate((('fwd', d.x, d.fwd), ('adj', d.gy, d.adj))):
        got = launch(kind, d.blk, v)[0]
        hold_to_bound(f'{cid} {kind}', got, ref, bound)
        err, base = max_rel_err(got, ref), CPU_BASE[cid][k]
        print(f'{cid} {kind} sharp: max |d| / max |ref| {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
        assert err <= FACTOR * base
        assert torch.equal(launch(kind, d.blk, v)[0], got), f'{cid} {kind}: two launches differ'


@gpu
@pytest.mark.parametrize('cid', [c.id for c in CASES if c.deltas])
def test_case_deltas(cid):
    d = case_data(cid)
    v, fwd, adj = delta_data(cid)
    blk = np.repeat(d.blk, v.shape[0])
    for kind, (ref, bound) in (('fwd', fwd), ('adj', adj)):
        got = launch(kind, blk, v, bias=0)
        assert bool((bound > 0).any())
        hold_to_bound(f'{cid} {kind} deltas', got, ref, bound)


def with_col(blk, m3, offset):
    out = blk.copy()
    col = np.concatenate([np.asarray(m3, np.float32).reshape(3, 3), np.asarray(offset, np.float32).reshape(3, 1)], 1)
    out['col'][:] = col.reshape(-1)
    return out


@gpu
@pytest.mark.parametrize('hw', SHAPES, ids=[f'{h}x{w}' for h, w in SHAPES])
def test_mixed_pad_batch_and_colour_invariants(hw):
    """One launch over the entries of every case of this (H, W): the pads differ per sample."""
    cases = [c for c in CASES if (c.H, c.W) == hw]
    data = [case_data(c.id) for c in cases]
    blk = np.concatenate([d.blk for d in data])
    assert len({d.pads for d in data}) > 1 or all(max(d.pads) == 0 for d in data)      # 7-pixel images admit pad 0 only
    x, gy = torch.stack([d.x for d in data]), torch.stack([d.gy for d in data])
    fwd, adj = launch('fwd', blk, x), launch('adj', blk, gy)
    assert torch.equal(launch('fwd', blk, x), fwd) and torch.equal(launch('adj', blk, gy), adj), 'two launches differ'
    for n, (c, d) in enumerate(zip(cases, data)):
        assert torch.equal(launch('fwd', d.blk, d.x)[0], fwd[n]), f'{c.id}: forward alone differs from the batch'
        assert torch.equal(launch('adj', d.blk, d.gy)[0], adj[n]), f'{c.id}: adjoint alone differs from the batch'
    eye, zero, off = np.eye(3), np.zeros(3), np.array([0.25, -1.5, 3.0])
    ident = launch('fwd', with_col(blk, eye, zero), x, bias=0)
    assert torch.equal(launch('fwd', with_col(blk, eye, zero), x, bias=1), ident), 'identity colour: bias = 1 with a zero offset'
    assert torch.equal(launch('fwd', with_col(blk, eye, off), x, bias=0), ident), 'bias = 0 does not ignore the offset'
    assert torch.equal(launch('fwd', with_col(blk, eye, off), x, bias=1), ident + torch.tensor(off).float().view(1, 3, 1, 1))
    adj_ident = launch('adj', with_col(blk, eye, off), gy)
    for perm in ((1, 2, 0), (0, 2, 1), (2, 1, 0)):
        pm = eye[list(perm)]                                              # out[i] = d[perm[i]]
        assert torch.equal(launch('fwd', with_col(blk, pm, zero), x, bias=1), ident[:, list(perm)]), f'forward, permutation {perm}'
        inv = [perm.index(k) for k in range(3)]                          # g_region[perm[c]] = acc[c]: gx[k] is the identity-colour gx[inv[k]]
        assert torch.equal(launch('adj', with_col(blk, pm, zero), gy), adj_ident[:, inv]), f'adjoint, permutation {perm}'
    const = launch('fwd', with_col(blk, np.zeros((3, 3)), off), x, bias=1)
    assert torch.equal(const, torch.tensor(off).float().view(1, 3, 1, 1).expand_as(const).contiguous()), 'col[:, :3] = 0'


# ---------------------------------------------------------------------------------------------------------- refusals
@gpu
def test_refused_calls_return_22_and_write_nothing():
    from rick_amd._lib import lib
    d = case_data('id-7x9')
    N, H, W = 2, 7, 9
    src, ws, dst = Fenced(N * 3 * H * W), Guarded(lib.rick_augment_workspace_floats(N, H, W)), Guarded(N * 3 * H * W)
    src.v.fill_(1.0)
    buf, prm = param_buffer(np.repeat(d.blk, N))

    def call(kind, a='', pr='', w='', b='', n=N, h=H, wd=W):
        a, pr, w, b = (dflt if v == '' else v for v, dflt in ((a, p(src)), (pr, prm), (w, p(ws)), (b, p(dst))))
        if kind == 'fwd':
            return lib.rick_augment_fwd_f32(a, pr, w, b, n, h, wd, 1, stream())
        return lib.rick_augment_adj_f32(a, pr, w, b, n, h, wd, stream())

    count = 0
    for kind in ('fwd', 'adj'):
        calls = {'in = NULL': call(kind, a=None), 'params = NULL': call(kind, pr=None), 'ws = NULL': call(kind, w=None),
                 'out = NULL': call(kind, b=None), 'N = 0': call(kind, n=0), 'N = -1': call(kind, n=-1), 'H = 6': call(kind, h=6),
                 'W = 6': call(kind, wd=6), 'H = 16385': call(kind, h=16385), 'W = 16385': call(kind, wd=16385)}
        torch.cuda.synchronize()
        for what, rc in calls.items():
            assert rc == EINVAL, f'{kind}: {what}: status {rc}'
        assert ws.untouched() and dst.untouched(), f'{kind}: a refused call wrote'
        count += len(calls)
    assert lib.rick_augment_workspace_floats(0, H, W) == lib.rick_augment_workspace_floats(N, 0, W) == -1
    assert lib.rick_augment_workspace_floats(N, H, 0) == -1
    assert call('fwd') == 0 and call('adj') == 0                           # the same buffers are accepted as they are
    torch.cuda.synchronize()
    ws.assert_bands('workspace')
    dst.assert_bands('output')
    print(f'refusals: {count} calls returned 22 and wrote nothing')
