"""Every dispatch form of the convolution weight gradient (rick_amd/csrc/wgrad.hip), through the C ABI with a hand-built
ConvGeom, against the fp64 expression written out here:

    gw[co*s_co + ci*s_ci + wt[t]*s_t]  (+)=  alpha * sum_n sum_(py,px in GH x GW)
            (ascale[n,co] * gy[n,py,px,co]) * (bscale[n,ci] * x[n, py*is+dy[t], px*is+dx[t], ci])      (x = 0 outside IH x IW)

The launcher is replayed on the host (make_tiling, wgrad_plan, the LDS budgets, wgrad_fast, the branch order of launch_wgrad,
the block mapping at the top of the kernels, the second-stage choice of wgrad_run); every case states the form it reaches as a
literal (`want`), which is also its id, and the host-only test holds the literal to the replay and the replay to the library
(rick_conv_wgrad_workspace_bytes, rick_conv_wgrad_split_supported).

Checks, none with a measured tolerance:

  exact11  both operands non-zero integers |v| <= 4 of mixed sign, scales in {0.5, 1, 2}, alpha = 0.25, and
           sum |terms| < 2**24 units for every output element (asserted on the CPU).  Every operand fits fp16's 11 bits after
           the power-of-two operand exponent (conv_common.h), so `lo` is zero and every product and partial sum is an exact
           fp32 number in any order, through split-K and the second stage: the device result is torch.equal to the fp64
           result cast to fp32.  Pins indexing, halos, masks, tails, tap-to-slice mapping and the reductions.
  exact22g / exact22x  (split == 2) one operand (gy / x) takes sign * (k + m * 2**-10), k in {2, 3}, m in {1, 3}: 12
           significant bits with the last one set, so hi != v and lo != 0; the other operand small integers.  hi*hi + lo*hi is
           exact in units of 2**-10 and lo*lo is identically zero (the other operand's lo is): torch.equal again.  A form that
           drops or misplaces the `lo` half of either operand fails here and nowhere in exact11.
  bound    standard-normal operands, scales in [0.5, 1.5]; per output element |dev - ref64| <= the sum of (bound_of):
             3 * 2**-22 * S                     representation: |v - hi - lo| <= 2**-22 |v| on either operand (conv_common.h), and
                                                the dropped lo*lo <= 2**-22 |term|   (split == 1: 2 * 2**-11 * S, two operands
                                                rounded to 11 bits);  S = sum |terms| (+ |old|)
             2**-27 * (Amax sum|b| + Bmax sum|a|)   values below the 32x window of the exponent: absolute error 2**-27 of the
                                                operand maximum each, times the other operand
             (n + nsplit + K) * 2**-24 * S      fp32 accumulation in any order: n positions, nsplit partial tiles, and K = 6 further
                                                roundings on a term: the two scale products, two more additions (three MFMA
                                                products per term), alpha, the accumulation into the old value
             2**-23 |ref|                       one ulp of the result
           The host-only test emulates the split with a tensor-wide exponent and shows that the representation part is not
           tighter than the method.  A bound case is launched twice: bit-identical (fixed summation order, no atomics).
           The accumulation part grows with n: at the batches of 113 the non-pipelined forms need on 8 x 8 grids (n = 7 232) the
           bound no longer sees a lost lo half, so those forms also run on 4 x 4 grids, where exact22 fits its budget.

Every device case: output and workspace between sentinel bands; output elements the launch does not name (gaps of the layout,
slices outside a tap subset, everything when the call is refused) keep the sentinel or the old value bit for bit; the operands,
scale tables and split-image headers are views into buffers that hold NaN on either side; the saturation counter stays put.

Forms no valid geometry reaches (production build, so they have no case): the four-wave whole-tile kernel at NT in {1, 9}
with one image per tile and fp32 or two split-image operands — conv_wgrad8_kernel takes those calls, its own LDS test
(wgrad8_lds_bytes) being the pipelined budget wgrad_fast has already passed; the instantiations themselves run with several
images per tile (4 x 4 grids) and with one split-image operand.  The third block mapping's `debug` arm and the RICK_WGRAD8 /
RICK_WGRAD_NOPIPE / RICK_WR_TILE switches exist in the experiment build only.
"""
import ctypes
import math
import types

import pytest
import torch

from rick_amd.synth import synth_tensor
from tests.forms_common import (SENT, Fenced, Guarded, cdiv, f32, fenced, fine, ilog2_ceil, ints, p, sat_count, scales,
                                split_image, stream)

gpu = pytest.mark.gpu
EINVAL = 22
LDS_MAX = 160 * 1024
K_ROUND = 6                   # extra roundings on a term (module docstring)


def case(**kw):
    return types.SimpleNamespace(**kw)


# ---------------------------------------------------------------------------------------------------------- geometries
def _k3(s):
    return [(ky - (1 if s == 1 else 0), kx - (1 if s == 1 else 0), ky * 3 + kx) for ky in range(3) for kx in range(3)]


# kind -> (input stride, input extent of a grid extent, taps (dy, dx, slice), slices)
KINDS = {
    'k3': (1, lambda n: n, _k3(1), 9),                                        # 3 x 3, stride 1, pad 1
    'k1': (1, lambda n: n, [(0, 0, 0)], 1),                                   # 1 x 1
    'k3s2': (2, lambda n: 2 * n + 1, _k3(2), 9),                              # 3 x 3, stride 2, pad 0
    'k1s2': (2, lambda n: 2 * n - 1, [(0, 0, 0)], 1),                         # 1 x 1, stride 2
    'k2': (1, lambda n: n + 1, [(ky, kx, ky * 2 + kx) for ky in range(2) for kx in range(2)], 4),       # 2 x 2, pad 0
    'k2s2': (2, lambda n: 2 * n, [(ky, kx, ky * 2 + kx) for ky in range(2) for kx in range(2)], 4),     # 2 x 2, stride 2
    'c4of9': (1, lambda n: n, [(-1, -1, 0), (-1, 1, 2), (1, -1, 6), (1, 1, 8)], 9),   # the corners of 3 x 3: a tap subset
    'r3of9': (1, lambda n: n, [(0, -1, 3), (0, 0, 4), (0, 1, 5)], 9),         # the middle row: three taps on the NT = 4 kernels
    'k10': (1, lambda n: n, _k3(1) + [(0, 2, 9)], 10),                        # ten taps: refused
    'k3s3': (3, lambda n: 3 * n, [(ky, kx, ky * 3 + kx) for ky in range(3) for kx in range(3)], 9),     # stride 3: patch too large
}


def make_geom(c, alpha=0.25):
    from rick_amd._lib import ConvGeom
    is_, ext, taps, nsl = KINDS[c.kind]
    g = ConvGeom()
    g.N, g.IH, g.IW, g.Ci = c.N, ext(c.GH), ext(c.GW), c.Ci
    g.OH, g.OW, g.Co, g.GH, g.GW = c.GH, c.GW, c.Co, c.GH, c.GW
    g.is_, g.os, g.oy0, g.ox0 = is_, 1, 0, 0
    g.ntaps, g.nslices = len(taps), nsl
    for t, (dy, dx, wt) in enumerate(taps):
        g.dy[t], g.dx[t], g.wt[t] = dy, dx, wt
    g.split, g.alpha = c.split, alpha
    return g


# ------------------------------------------------------------------------------------------ host-side launcher replay
def make_tiling(g, tile=64):
    """conv_tiling.h make_tiling(g, 64, ..): the fields the weight gradient uses."""
    tl = ilog2_ceil(tile)
    tw = ilog2_ceil(g.GW)
    tw = min(tw, 4)
    tw = max(tw, 2)
    tw = min(tw, tl)
    th = min(ilog2_ceil(g.GH), tl - tw)
    t = types.SimpleNamespace(tw=tw, th=th, nb=tile >> (tw + th))
    t.nbe = min(t.nb, g.N)
    t.ntx, t.nty, t.ntn = cdiv(g.GW, 1 << tw), cdiv(g.GH, 1 << th), cdiv(g.N, t.nbe)
    dys, dxs = [g.dy[i] for i in range(g.ntaps)], [g.dx[i] for i in range(g.ntaps)]
    t.PH = ((1 << th) - 1) * g.is_ + (max(dys) - min(dys)) + 1
    t.PW = ((1 << tw) - 1) * g.is_ + (max(dxs) - min(dxs)) + 1
    t.NPP = t.nbe * t.PH * t.PW
    t.nchunks, t.ncot = cdiv(g.Ci, 32), cdiv(g.Co, 128)
    t.ntiles = t.ntx * t.nty * t.ntn
    return t


def wgrad_plan(g):
    """-> (tiling, nsplit, tiles per split): minimise 2 * waves * (tiles + 8) + splits, multiples of 8 splits win ties."""
    t = make_tiling(g)
    cc = t.ncot * t.nchunks
    best_tps, best_cost = t.ntiles, 1 << 30
    for s in range(1, min(t.ntiles, 64) + 1):
        tp = cdiv(t.ntiles, s)
        se = cdiv(t.ntiles, tp)
        cost = 2 * cdiv(cc * se, 256) * (tp + 8) + se - (1 if se % 8 == 0 else 0)
        if cost < best_cost:
            best_cost, best_tps = cost, tp
    return t, cdiv(t.ntiles, best_tps), best_tps


def wgrad_lds_bytes(g, t, pipe):
    buf = 2 * 16384 + 2 * (t.NPP + 1) * 64
    return (2 if pipe else 1) * buf + ((t.NPP + 3) & ~3) * 4 + g.N * (128 + 32) * 4


wgrad8_lds_bytes = lambda g, t: wgrad_lds_bytes(g, t, True)      # the same expression in the source


def is_vec(g):
    return (g.Ci | g.Co) & 3 == 0


def wgrad_use_pipe(g, t):
    return g.split == 2 and is_vec(g) and wgrad_lds_bytes(g, t, True) <= LDS_MAX


def nt_of(g):
    return 1 if g.ntaps == 1 else 4 if g.ntaps <= 4 else 9


def wgrad_fast(g, t, NT):
    return (wgrad_use_pipe(g, t) and g.ntaps == NT and g.N * g.IH * g.IW * g.Ci < 1 << 29 and g.N * g.OH * g.OW * g.Co < 1 << 29
            and g.Co % 128 == 0 and g.Ci % 32 == 0 and g.GH % (1 << t.th) == 0 and g.GW % (1 << t.tw) == 0
            and g.N % t.nbe == 0 and t.nb == t.nbe)


def block_map(nsplit, ncc):
    """The branch at the top of both kernels: -> (name, [(split, cc) of block 0, 1, ..])."""
    nwg = nsplit * ncc
    if nsplit % 8 == 0:
        spx = nsplit >> 3
        return 'map1', [((b & 7) + 8 * ((b >> 3) % spx), (b >> 3) // spx) for b in range(nwg)]
    if nsplit in (1, 2, 4) and ncc % (8 // nsplit) == 0:
        xps = 8 // nsplit
        return 'map2', [((b & 7) // xps, ((b & 7) % xps) * (ncc // xps) + (b >> 3)) for b in range(nwg)]
    return 'map3', [(b // ncc, b % ncc) for b in range(nwg)]


def reduce_form(g, t, s_co, s_ci, s_t):
    nsl = g.nslices
    tile_reduce = t.ncot * t.nchunks >= 32
    if tile_reduce and s_t == 1 and s_ci == nsl and s_co >= g.Ci * nsl and nsl <= 16:
        return 'tile'
    if tile_reduce and s_t == 1 and s_co == nsl and s_ci >= g.Co * nsl and nsl <= 16:
        return 'tileT'
    return 'elem'


def replay(g, scaled, pk, strides):
    """wgrad_run + launch_wgrad<NT> for valid pointers: rc, the kernel instantiation, plan, block mapping, second stage."""
    t, nsplit, tps = wgrad_plan(g)
    NT = nt_of(g)
    r = types.SimpleNamespace(t=t, NT=NT, nsplit=nsplit, tps=tps, rc=0, branch=None,
                              ws_floats=nsplit * t.ncot * t.nchunks * g.ntaps * 128 * 32)
    r.map = block_map(nsplit, t.ncot * t.nchunks)[0]
    r.reduce = reduce_form(g, t, *strides)
    vec, small, pipe, fast = is_vec(g), t.NPP <= 128, wgrad_use_pipe(g, t), wgrad_fast(g, t, NT)
    r.fast, r.pipe, r.small = fast, pipe, small
    if g.ntaps > 9:
        r.rc, r.why = EINVAL, 'ntaps'
    elif wgrad_lds_bytes(g, t, False) > LDS_MAX:
        r.rc, r.why = EINVAL, 'lds'
    elif t.NPP > 384 or t.PH > 1023 or t.PW > 1023:
        r.rc, r.why = EINVAL, 'npp'
    elif g.split == 1 and not vec:
        r.rc, r.why = EINVAL, 'split1-novec'
    elif pk and (not fast or g.split != 2):
        r.rc, r.why = EINVAL, 'split-image'
    if r.rc:
        return r
    w8 = NT in (1, 9) and t.nbe == 1 and wgrad8_lds_bytes(g, t) <= LDS_MAX

    def k(split, v, pm, pp, f=0, pkk=0):
        return f'k<s{split},{"vec" if v else "novec"},pm{pm},{"pipe" if pp else "nopipe"},f{f},pk{pkk}>'
    if pk:
        r.branch = f'w8<pm{2 if small else 6},f1,pk3>' if pk == 3 and w8 else k(2, True, 4 if small else 12, True, 1, pk)
    elif fast and vec and g.split == 2 and w8:
        r.branch = f'w8<pm{2 if small else 6},f{2 if scaled else 1},pk0>'
    elif g.split == 1 and vec:
        r.branch = k(1, True, 12, False)
    elif not vec:
        r.branch = k(2, False, 12, False)
    elif fast:
        r.branch = k(2, True, 4 if small else 12, True, 2 if scaled else 1)
    else:
        r.branch = k(2, True, 4 if small else 12, pipe)
    return r


def split_supported(g):
    """rick_conv_wgrad_split_supported: the whole-tile form with at most 384 patch pixels."""
    if g.ntaps > 9 or g.split != 2:
        return 0
    t = make_tiling(g)
    return int(t.NPP <= 384 and wgrad_fast(g, t, nt_of(g)))


def strides_of(c, g):
    """-> (s_co, s_ci, s_t) of the destination layout: 'co' [co][ci][slice] (+ `gap` floats per co row), 'ci' [ci][co][slice],
    'st' [slice][co][ci] (a general s_t)."""
    nsl = g.nslices
    if c.lay == 'co':
        return g.Ci * nsl + c.gap, nsl, 1
    if c.lay == 'ci':
        return nsl, g.Co * nsl + c.gap, 1
    return g.Ci + c.gap, 1, g.Co * (g.Ci + c.gap)


def want_of(c):
    g = make_geom(c)
    r = replay(g, bool(c.sc), c.pk, strides_of(c, g))
    return r, (f'{r.branch}/NT{r.NT}/s{r.nsplit}x{r.tps}/{r.map}/{r.reduce}' if r.rc == 0 else f'EINVAL:{r.why}')


# ------------------------------------------------------------------------------------------------------- case table
def W(kind, N, Co, Ci, GH, GW, want, split=2, sc='', pk=0, lay='co', gap=0, acc=0, e22=False):
    """One case; `want` is the literal 'kernel<..>/NT/s<splits>x<tiles per split>/mapping/second stage' it must reach.
    sc: which of ascale ('a') / bscale ('b') are given; pk: bit 0 = gy, bit 1 = x is a split image; e22: runs exact22 too."""
    tag = f'{kind}-N{N}-Co{Co}-Ci{Ci}-{GH}x{GW}' + (f'-split{split}' if split != 2 else '') + (f'-sc:{sc}' if sc else '') + \
          (f'-lay:{lay}' if lay != 'co' else '') + (f'-gap{gap}' if gap else '') + ('-acc' if acc else '')
    return case(id=want + '-' + tag, want=want, kind=kind, N=N, Co=Co, Ci=Ci, GH=GH, GW=GW, split=split, sc=sc, pk=pk, lay=lay,
                gap=gap, acc=acc, e22=e22)


CASES = [
    # the simplest form first: one tile, one split, guarded scalar loads, no pipeline
    W('k3', 1, 10, 6, 8, 8, 'k<s2,novec,pm12,nopipe,f0,pk0>/NT9/s1x1/map3/elem', e22=True),
    # 1. the eight-wave form
    W('k3', 1, 128, 32, 8, 8, 'w8<pm2,f1,pk0>/NT9/s1x1/map3/elem', e22=True),
    W('k3', 5, 128, 32, 8, 8, 'w8<pm2,f2,pk0>/NT9/s3x2/map3/elem', sc='ab', e22=True),
    W('k3', 4, 256, 64, 8, 8, 'w8<pm2,f1,pk3>/NT9/s2x2/map2/elem', pk=3, e22=True),
    W('k3', 4, 128, 32, 16, 16, 'w8<pm2,f1,pk0>/NT9/s8x2/map1/elem'),
    W('k1', 1, 128, 32, 8, 8, 'w8<pm2,f1,pk0>/NT1/s1x1/map3/elem'),
    W('k1', 3, 128, 32, 8, 8, 'w8<pm2,f2,pk0>/NT1/s3x1/map3/elem', sc='a'),
    W('k1', 2, 256, 64, 8, 8, 'w8<pm2,f1,pk3>/NT1/s2x1/map2/elem', pk=3),
    W('k3s2', 1, 128, 32, 8, 8, 'w8<pm6,f1,pk0>/NT9/s1x1/map3/elem'),
    W('k3s2', 3, 128, 32, 8, 8, 'w8<pm6,f2,pk0>/NT9/s3x1/map3/elem', sc='b', e22=True),
    W('k3s2', 2, 128, 32, 8, 8, 'w8<pm6,f1,pk3>/NT9/s2x1/map3/elem', pk=3, e22=True),
    W('k1s2', 1, 128, 32, 8, 8, 'w8<pm6,f1,pk0>/NT1/s1x1/map3/elem'),
    W('k1s2', 2, 128, 32, 8, 8, 'w8<pm6,f2,pk0>/NT1/s2x1/map3/elem', sc='ab'),
    W('k1s2', 3, 128, 32, 8, 8, 'w8<pm6,f1,pk3>/NT1/s3x1/map3/elem', pk=3),
    # 2. split-image forms of conv_wgrad_kernel
    W('k3', 2, 128, 32, 8, 8, 'k<s2,vec,pm4,pipe,f1,pk1>/NT9/s2x1/map3/elem', pk=1, e22=True),
    W('k3', 1, 128, 64, 16, 16, 'k<s2,vec,pm4,pipe,f1,pk2>/NT9/s2x2/map3/elem', pk=2, e22=True),
    W('k3s2', 1, 128, 32, 8, 8, 'k<s2,vec,pm12,pipe,f1,pk1>/NT9/s1x1/map3/elem', pk=1),
    W('k3s2', 2, 128, 32, 8, 8, 'k<s2,vec,pm12,pipe,f1,pk2>/NT9/s2x1/map3/elem', pk=2),
    W('k3', 4, 128, 32, 4, 4, 'k<s2,vec,pm12,pipe,f1,pk3>/NT9/s1x1/map3/elem', pk=3, e22=True),
    W('k1', 8, 128, 32, 4, 4, 'k<s2,vec,pm4,pipe,f1,pk3>/NT1/s2x1/map3/elem', pk=3),
    # 3. plain fp16 (split == 1)
    W('k3', 1, 128, 32, 8, 8, 'k<s1,vec,pm12,nopipe,f0,pk0>/NT9/s1x1/map3/elem', split=1),
    W('k3', 3, 192, 48, 8, 12, 'k<s1,vec,pm12,nopipe,f0,pk0>/NT9/s3x2/map3/elem', split=1),
    # 4. channel counts that are no multiple of 4
    W('k3', 3, 130, 32, 8, 12, 'k<s2,novec,pm12,nopipe,f0,pk0>/NT9/s3x2/map3/elem'),
    W('k1', 2, 128, 6, 4, 4, 'k<s2,novec,pm12,nopipe,f0,pk0>/NT1/s1x1/map3/elem'),
    # 5. whole-tile forms outside the eight-wave kernel: several images per tile, four taps
    W('k3', 4, 128, 32, 4, 4, 'k<s2,vec,pm12,pipe,f1,pk0>/NT9/s1x1/map3/elem', e22=True),
    W('k3', 8, 128, 32, 4, 4, 'k<s2,vec,pm12,pipe,f2,pk0>/NT9/s2x1/map3/elem', sc='ab', e22=True),
    W('k1', 4, 128, 32, 4, 4, 'k<s2,vec,pm4,pipe,f1,pk0>/NT1/s1x1/map3/elem'),
    W('k1', 8, 256, 32, 4, 4, 'k<s2,vec,pm4,pipe,f2,pk0>/NT1/s2x1/map3/elem', sc='b'),
    W('k2', 1, 128, 32, 8, 8, 'k<s2,vec,pm4,pipe,f1,pk0>/NT4/s1x1/map3/elem'),
    W('k2', 2, 128, 32, 8, 8, 'k<s2,vec,pm4,pipe,f2,pk0>/NT4/s2x1/map3/elem', sc='a', e22=True),
    W('k2s2', 1, 128, 32, 8, 8, 'k<s2,vec,pm12,pipe,f1,pk0>/NT4/s1x1/map3/elem'),
    W('k2s2', 3, 128, 32, 8, 8, 'k<s2,vec,pm12,pipe,f2,pk0>/NT4/s3x1/map3/elem', sc='ab'),
    W('c4of9', 2, 128, 32, 8, 8, 'k<s2,vec,pm4,pipe,f1,pk0>/NT4/s2x1/map3/elem', acc=1),
    # 6. ragged, pipelined
    W('k3', 2, 192, 32, 8, 8, 'k<s2,vec,pm4,pipe,f0,pk0>/NT9/s2x1/map3/elem', e22=True),
    W('k3', 2, 128, 48, 8, 8, 'k<s2,vec,pm4,pipe,f0,pk0>/NT9/s2x1/map3/elem', sc='ab'),
    W('k3', 2, 128, 32, 18, 16, 'k<s2,vec,pm4,pipe,f0,pk0>/NT9/s5x2/map3/elem'),
    W('k3', 1, 128, 32, 8, 12, 'k<s2,vec,pm4,pipe,f0,pk0>/NT9/s2x1/map3/elem'),
    W('k3', 3, 128, 32, 4, 4, 'k<s2,vec,pm4,pipe,f0,pk0>/NT9/s1x1/map3/elem', e22=True),
    W('k3', 5, 128, 32, 4, 4, 'k<s2,vec,pm12,pipe,f0,pk0>/NT9/s2x1/map3/elem', sc='a'),
    W('k3s2', 2, 192, 48, 8, 8, 'k<s2,vec,pm12,pipe,f0,pk0>/NT9/s2x1/map2/elem'),
    W('k3s2', 1, 128, 32, 9, 9, 'k<s2,vec,pm12,pipe,f0,pk0>/NT9/s3x1/map3/elem', sc='b'),
    W('r3of9', 2, 128, 32, 8, 8, 'k<s2,vec,pm4,pipe,f0,pk0>/NT4/s2x1/map3/elem'),
    W('k1', 2, 192, 48, 8, 8, 'k<s2,vec,pm4,pipe,f0,pk0>/NT1/s2x1/map2/elem'),
    W('k2', 2, 128, 48, 8, 8, 'k<s2,vec,pm4,pipe,f0,pk0>/NT4/s2x1/map3/elem'),
    # 7. ragged, not pipelined: the batch leaves LDS for one operand buffer only
    W('k3', 113, 128, 32, 8, 8, 'k<s2,vec,pm4,nopipe,f0,pk0>/NT9/s13x9/map3/elem'),
    W('k3', 113, 128, 32, 8, 8, 'k<s2,vec,pm4,nopipe,f0,pk0>/NT9/s13x9/map3/elem', sc='ab'),
    W('k3s2', 36, 128, 32, 8, 8, 'k<s2,vec,pm12,nopipe,f0,pk0>/NT9/s8x5/map1/elem'),
    W('k3s2', 36, 128, 32, 8, 8, 'k<s2,vec,pm12,nopipe,f0,pk0>/NT9/s8x5/map1/elem', sc='ab'),
    # ... on 4 x 4 grids, where the batch that overflows LDS still leaves few enough positions for the exact22 budget (the
    # bound is loose at n = 7 232: it does not see a lost lo half there)
    W('k1', 130, 128, 32, 4, 4, 'k<s2,vec,pm4,nopipe,f0,pk0>/NT1/s7x5/map3/elem', e22=True),
    W('k3', 116, 128, 32, 4, 4, 'k<s2,vec,pm12,nopipe,f0,pk0>/NT9/s8x4/map1/elem', e22=True),
    # 9. second stage: the two tile forms (>= 32 (co tile, chunk) tiles), the element form, a general s_t, tap subsets
    W('k3', 1, 512, 256, 8, 8, 'w8<pm2,f1,pk0>/NT9/s1x1/map2/tile'),
    W('k3', 1, 512, 256, 8, 8, 'w8<pm2,f1,pk0>/NT9/s1x1/map2/tile', acc=1, gap=5),
    W('k3', 1, 512, 256, 8, 8, 'w8<pm2,f1,pk0>/NT9/s1x1/map2/tileT', lay='ci'),
    W('k3', 1, 512, 256, 8, 8, 'w8<pm2,f1,pk0>/NT9/s1x1/map2/tileT', lay='ci', acc=1, gap=7),
    W('k3', 2, 500, 264, 8, 8, 'k<s2,vec,pm4,pipe,f0,pk0>/NT9/s2x1/map2/tile', sc='ab'),
    W('k3', 2, 500, 264, 8, 8, 'k<s2,vec,pm4,pipe,f0,pk0>/NT9/s2x1/map2/tileT', lay='ci', acc=1),
    W('c4of9', 1, 512, 256, 8, 8, 'k<s2,vec,pm4,pipe,f1,pk0>/NT4/s1x1/map2/tile', acc=1),
    W('c4of9', 1, 512, 256, 8, 8, 'k<s2,vec,pm4,pipe,f1,pk0>/NT4/s1x1/map2/tileT', lay='ci'),
    W('c4of9', 1, 512, 256, 8, 8, 'k<s2,vec,pm4,pipe,f1,pk0>/NT4/s1x1/map2/tileT', lay='ci', acc=1),
    W('k1', 1, 512, 256, 8, 8, 'w8<pm2,f1,pk0>/NT1/s1x1/map2/tile', acc=1),
    W('k1', 1, 512, 256, 8, 8, 'w8<pm2,f1,pk0>/NT1/s1x1/map2/tileT', lay='ci'),
    W('k3', 2, 128, 32, 8, 8, 'w8<pm2,f1,pk0>/NT9/s2x1/map3/elem', lay='st'),
    W('k3', 2, 192, 48, 8, 8, 'k<s2,vec,pm4,pipe,f0,pk0>/NT9/s2x1/map2/elem', lay='st', acc=1, gap=2),
    W('k3', 3, 128, 64, 8, 8, 'w8<pm2,f1,pk0>/NT9/s3x1/map3/elem', acc=1),
    W('c4of9', 2, 128, 32, 8, 8, 'k<s2,vec,pm4,pipe,f1,pk0>/NT4/s2x1/map3/elem', lay='st'),
]
# 10. refused before anything is launched (the pointer gates: test_wgrad_refuses_bad_pointers_and_headerless_split_calls)
GATES = [
    W('k3s3', 1, 128, 32, 4, 16, 'EINVAL:npp'),                        # 12 x 48 patch pixels > 384
    W('k3', 184, 128, 32, 8, 8, 'EINVAL:lds'),                         # one operand buffer + 184 * 160 scale floats > 160 KB
    W('k10', 1, 128, 32, 8, 8, 'EINVAL:ntaps'),
    W('k3', 1, 10, 6, 8, 8, 'EINVAL:split1-novec', split=1),
    W('k3', 2, 192, 48, 8, 8, 'EINVAL:split-image', pk=3),             # ragged channels: rick_conv_wgrad_split_supported says no
    W('k3', 1, 128, 32, 8, 8, 'EINVAL:split-image', pk=1, split=1),
]


def params(pairs):
    return pytest.mark.parametrize('c,mode', pairs, ids=[f'{c.id}-{m}' for c, m in pairs])


def modes_of(c):
    return ('exact11', 'bound') + (('exact22g', 'exact22x') if c.e22 else ())


DEVICE = [(c, m) for c in CASES for m in modes_of(c)]


# ----------------------------------------------------------------------------------------------------------- inputs
def shifted(c, B, dy, dx):
    """B [N, IH, IW, Ci] -> [N, GH, GW, Ci]: B[n, py*is + dy, px*is + dx], zero outside the input."""
    is_ = KINDS[c.kind][0]
    IH, IW = B.shape[1], B.shape[2]
    iy, ix = torch.arange(c.GH) * is_ + dy, torch.arange(c.GW) * is_ + dx
    ok = ((iy >= 0) & (iy < IH))[:, None] & ((ix >= 0) & (ix < IW))[None, :]
    return B[:, iy.clamp(0, IH - 1)][:, :, ix.clamp(0, IW - 1)] * ok[None, :, :, None].to(B.dtype)


def contract(c, A, B):
    """sum over (n, py, px) of A[n,py,px,co] * B[n, py*is+dy[t], px*is+dx[t], ci] -> [Co, Ci, ntaps] (fp64)."""
    taps = KINDS[c.kind][2]
    out = torch.empty(c.Co, c.Ci, len(taps), dtype=torch.float64)
    At = A.reshape(-1, c.Co).t().contiguous()
    for t, (dy, dx, _) in enumerate(taps):
        out[:, :, t] = At @ shifted(c, B, dy, dx).reshape(-1, c.Ci)
    return out


def build(c, mode):
    """Operands, the fp64 reference and the per-element sums the checks need, with the premises of the checks asserted."""
    is_, ext, taps, nsl = KINDS[c.kind]
    N, Co, Ci, GH, GW, IH, IW = c.N, c.Co, c.Ci, c.GH, c.GW, ext(c.GH), ext(c.GW)
    exact = mode != 'bound'
    alpha = 0.25 if exact else f32(1 / math.sqrt(2))
    if mode == 'bound':
        gy, x = synth_tensor('wgf/' + c.id + '/gy', (N, GH, GW, Co)), synth_tensor('wgf/' + c.id + '/x', (N, IH, IW, Ci))
    elif mode == 'exact11':
        gy, x = ints(c.id + '/gy', (N, GH, GW, Co), 4), ints(c.id + '/x', (N, IH, IW, Ci), 4)
    elif mode == 'exact22g':
        gy, x = fine(c.id + '/gy', (N, GH, GW, Co)), ints(c.id + '/x', (N, IH, IW, Ci), 2)
    else:
        gy, x = ints(c.id + '/gy', (N, GH, GW, Co), 2), fine(c.id + '/x', (N, IH, IW, Ci))
    asc = scales(c.id + '/asc', (N, Co), mode) if 'a' in c.sc else None
    bsc = scales(c.id + '/bsc', (N, Ci), mode) if 'b' in c.sc else None
    assert not (c.pk and c.sc), 'a split image has its scales folded in'
    A = gy.double() * (asc.double()[:, None, None, :] if asc is not None else 1.0)
    B = x.double() * (bsc.double()[:, None, None, :] if bsc is not None else 1.0)
    b = types.SimpleNamespace(gy=gy, x=x, asc=asc, bsc=bsc, alpha=alpha, n=N * GH * GW, g=make_geom(c, alpha))
    b.ref = alpha * contract(c, A, B)
    b.S = alpha * contract(c, A.abs(), B.abs())
    # the window term: Amax * sum |b| + Bmax * sum |a| over the terms of an element
    sa = A.abs().reshape(-1, Co).sum(0)
    sb = torch.stack([shifted(c, B.abs(), dy, dx).reshape(-1, Ci).sum(0) for dy, dx, _ in taps], 1)         # [Ci, ntaps]
    b.Wn = alpha * (float(A.abs().max()) * sb[None, :, :] + float(B.abs().max()) * sa[:, None, None])
    b.unit = alpha * (0.5 if asc is not None else 1.0) * (0.5 if bsc is not None else 1.0) * (1.0 if mode in ('exact11', 'bound') else 2.0 ** -10)
    # destination: strides, the flat index of every element the launch names, the buffer's contents before the launch
    b.strides = s_co, s_ci, s_t = strides_of(c, b.g)
    wt = torch.tensor([w for _, _, w in taps])
    b.idx = (torch.arange(Co)[:, None, None] * s_co + torch.arange(Ci)[None, :, None] * s_ci + wt[None, None, :] * s_t).reshape(-1)
    b.span = (Co - 1) * s_co + (Ci - 1) * s_ci + (nsl - 1) * s_t + 1
    assert torch.unique(b.idx).numel() == b.idx.numel() and int(b.idx.max()) < b.span
    if c.acc:
        b.before = ints(c.id + '/old', (b.span,), 50) if exact else synth_tensor('wgf/' + c.id + '/old', (b.span,))
        b.old = b.before.double()[b.idx].reshape(b.ref.shape)
        b.ref, b.S = b.ref + b.old, b.S + b.old.abs()
    else:
        b.before, b.old = torch.full((b.span,), SENT), 0.0
    # the premises
    if exact:
        assert float(b.S.max()) / b.unit < 2 ** 24, f'{c.id}: sum |terms| = {float(b.S.max()) / b.unit} units: not exact in fp32'
        assert torch.equal(b.ref.float().double(), b.ref) and not bool((b.ref == SENT).any())
    for name, v, C in (('gy', gy, Co), ('x', x, Ci)):
        cols = v.reshape(-1, C).t()
        assert float(v.min()) < 0 < float(v.max()), f'{name}: one sign only'
        assert torch.unique(cols, dim=0).shape[0] == C, f'{name}: two equal channels'
        assert N == 1 or torch.unique(v.reshape(N, -1), dim=0).shape[0] == N, f'{name}: two equal images'
    for t in range(len(taps)):
        assert float(b.ref[:, :, t].min()) < float(b.ref[:, :, t].max()), 'constant output: the case cannot tell operands apart'
    return b


def bound_of(c, b, r):
    rep = (3 * 2.0 ** -22 if c.split == 2 else 2 * 2.0 ** -11) * b.S
    return rep + 2.0 ** -27 * b.Wn + (b.n + r.nsplit + K_ROUND) * 2.0 ** -24 * b.S + 2.0 ** -23 * b.ref.abs()


def emulate(c, b):
    """The documented split on the CPU with ONE exponent per operand (maximum placed in [4, 8), as CV_EXP_TARGET = 2):
    hi = fp16(v * 2^e), lo = fp16(v * 2^e - hi), products hi*hi + hi*lo + lo*hi (no lo*lo), summed in fp64."""
    def halves(v, sc):
        v = v * sc[:, None, None, :] if sc is not None else v           # (fp32, as the device forms it)
        e = 2 - math.floor(math.log2(float(v.abs().max())))
        w = v * 2.0 ** e
        hi = w.half()
        lo = (w - hi.float()).half() if c.split == 2 else torch.zeros_like(hi)
        return hi.double(), lo.double(), 2.0 ** -e
    ah, al, ua = halves(b.gy, b.asc)
    bh, bl, ub = halves(b.x, b.bsc)
    return b.alpha * ua * ub * (contract(c, ah, bh) + contract(c, ah, bl) + contract(c, al, bh)) + b.old


# ---------------------------------------------------------------------------------------------------- host-only tests
def _feat(c, r):
    """The coverage items one case reaches, named from the replay (REQUIRED below lists what the tables must reach together)."""
    f = {f'{r.branch}/NT{r.NT}', r.map, r.reduce + ('+acc' if c.acc else ''), f'split{c.split}'}
    t = r.t
    if r.branch.startswith('k<s2,vec') and ',f0,' in r.branch:
        kind = 'pipe' if ',pipe,' in r.branch else 'nopipe'
        f.add(f'ragged-{kind}-{"small" if r.small else "large"}' + ('-scaled' if c.sc else ''))
        if r.pipe:
            f |= {f'ragged:Co{c.Co}' if c.Co % 128 else '', f'ragged:Ci{c.Ci}' if c.Ci % 32 else '',
                  'ragged:GH18,N2' if (c.GH, c.N) == (18, 2) else '', 'ragged:GW' if c.GW % (1 << t.tw) else '',
                  'ragged:N%nbe' if c.N % t.nbe else '', 'ragged:N<nb' if t.nbe < t.nb else ''}
    if r.fast and not r.branch.startswith('w8') and not c.pk:
        f.add(f'whole:{"nbe>1" if t.nbe > 1 else "NT4"}-{"small" if r.small else "large"}-{"scaled" if c.sc else "plain"}')
    if r.nsplit == 1:
        f.add('one split')
    if t.ntiles % r.tps:
        f.add('short last split')
    if r.nsplit % 8 == 0:
        f.add('8k splits')
    if r.nsplit in (2, 4) and r.map == 'map2':
        f.add('map2 with 2 or 4 splits')
    if r.map == 'map3' and (r.nsplit == 3 or (r.nsplit == 2 and (t.ncot * t.nchunks) % 2)):
        f.add('map3 with 3 splits, or 2 and odd ncc')
    if r.reduce != 'elem' and (c.Co % 128 or c.Ci % 32):
        f.add(r.reduce + ' ragged')
    if c.lay == 'st':
        f.add('elem general s_t' + ('+acc' if c.acc else ''))
    if c.kind == 'c4of9':
        f.add('subset:' + r.reduce)
    if c.kind == 'c4of9' and r.NT == 4:
        f.add('NT4 as 4 of 9 slices')
    if c.e22:
        f.add('e22:' + r.branch.split('<')[0] + ':' + r.branch[:-1].split(',')[-2] + ':' + r.branch[:-1].split(',')[-1])
        if r.branch.startswith('k<s2,vec'):      # the staging paths of conv_wgrad_kernel: pipelined or not, one image per tile or several
            f.add(f'e22:k:{"pipe" if r.pipe else "nopipe"}:{"one image" if t.nbe == 1 else "images"}:' + r.branch[:-1].split(',')[-2])
    f.discard('')
    return f


def _k(pm, pp, f=0, pk=0, s=2, v='vec'):
    return f'k<s{s},{v},pm{pm},{pp},f{f},pk{pk}>'


REQUIRED = (
    # 1. the eight-wave form: small / large patches, plain / scaled / split images, one tap and nine
    {f'w8<pm{pm},{fp}>/NT{nt}' for pm in (2, 6) for fp in ('f1,pk0', 'f2,pk0', 'f1,pk3') for nt in (1, 9)}
    # 2. split-image forms of conv_wgrad_kernel: one image operand on a fast geometry (small, large); two with nbe > 1
    | {_k(pm, 'pipe', 1, pk) + '/NT9' for pm in (4, 12) for pk in (1, 2)} | {_k(12, 'pipe', 1, 3) + '/NT9', _k(4, 'pipe', 1, 3) + '/NT1'}
    # 3. / 4. plain fp16, non-vector channels
    | {_k(12, 'nopipe', s=1) + '/NT9', _k(12, 'nopipe', v='novec') + '/NT9', 'split1'}
    # 5. whole-tile forms outside the eight-wave kernel
    | {f'whole:{w}-{sz}-{sc}' for w in ('nbe>1', 'NT4') for sz in ('small', 'large') for sc in ('plain', 'scaled')} | {'NT4 as 4 of 9 slices'}
    # 6. / 7. ragged forms
    | {f'ragged-pipe-{sz}' for sz in ('small', 'large')} | {'ragged:Co192', 'ragged:Ci48', 'ragged:GH18,N2', 'ragged:GW', 'ragged:N%nbe', 'ragged:N<nb'}
    | {f'ragged-nopipe-{sz}{sc}' for sz in ('small', 'large') for sc in ('', '-scaled')}
    | {_k(4, 'pipe') + '/NT4', _k(4, 'pipe') + '/NT1'}
    # 8. split-K and the three block mappings
    | {'one split', 'short last split', '8k splits', 'map2 with 2 or 4 splits', 'map3 with 3 splits, or 2 and odd ncc', 'map1', 'map2', 'map3'}
    # 9. second stage
    | {f'{rf}{a}' for rf in ('tile', 'tileT', 'elem', 'elem general s_t') for a in ('', '+acc')} | {'tile ragged', 'tileT ragged'}
    | {'subset:tile', 'subset:tileT', 'subset:elem'}
    # exact22: each kernel template, FAST value and PK value
    | {'e22:w8:f1:pk0', 'e22:w8:f2:pk0', 'e22:w8:f1:pk3', 'e22:k:f0:pk0', 'e22:k:f1:pk0', 'e22:k:f2:pk0', 'e22:k:f1:pk1', 'e22:k:f1:pk2',
       'e22:k:f1:pk3'}
    # ... and each staging path of conv_wgrad_kernel: not pipelined, pipelined ragged / whole-tile with one image per tile and several
    | {'e22:k:nopipe:images:f0', 'e22:k:pipe:one image:f0', 'e22:k:pipe:images:f0', 'e22:k:pipe:one image:f2', 'e22:k:pipe:images:f2',
       'e22:k:pipe:images:f1', 'e22:k:pipe:one image:f1'})
REQUIRED_GATES = {'npp', 'lds', 'ntaps', 'split1-novec', 'split-image'}


def test_case_ids_replay_and_library_agree():
    """No device.  Every case's literal `want` is what the replayed launcher picks; the replay's plan and whole-tile test are
    the library's own (workspace bytes, split-image support); every block mapping deals each (split, tile) pair to exactly one
    block and every split gets at least one position tile; the tables reach the whole coverage list."""
    from rick_amd._lib import lib
    assert len({c.id for c in CASES + GATES}) == len(CASES + GATES)
    reached = set()
    for c in CASES + GATES:
        g = make_geom(c)
        r, want = want_of(c)
        assert want == c.want, f'{c.id}: the replay reaches {want}'
        assert lib.rick_conv_wgrad_workspace_bytes(ctypes.byref(g)) == r.ws_floats * 4 == r.nsplit * r.t.ncot * r.t.nchunks * g.ntaps * 128 * 32 * 4, c.id
        assert lib.rick_conv_wgrad_split_supported(ctypes.byref(g)) == split_supported(g) == int(bool(r.fast and r.t.NPP <= 384 and g.ntaps <= 9)), c.id
        ncc = r.t.ncot * r.t.nchunks
        name, blocks = block_map(r.nsplit, ncc)
        assert sorted(blocks) == [(s, q) for s in range(r.nsplit) for q in range(ncc)], f'{c.id}: {name} is not a bijection'
        assert (r.nsplit - 1) * r.tps < r.t.ntiles <= r.nsplit * r.tps, c.id
        if c in CASES:
            assert r.rc == 0, c.id
            reached |= _feat(c, r)
            assert not c.e22 or c.split == 2
        else:
            assert r.rc == EINVAL, c.id
            reached.add(r.why)
    assert not REQUIRED - reached, f'not reached: {sorted(REQUIRED - reached)}'
    assert not REQUIRED_GATES - reached, f'gates not reached: {sorted(REQUIRED_GATES - reached)}'
    assert len(DEVICE) <= 170


def test_exact_inputs_fit_and_the_bound_is_not_tighter_than_the_split():
    """No device.  Every exact-mode builder passes its own assertions (sum |terms| < 2**24 units, distinct channels and images,
    mixed signs, non-constant results).  On the small cases the CPU emulation of the documented split stays inside the
    representation part of the bound alone — 3 * 2**-22 * S (split == 1: 2 * 2**-11 * S) — so that part is no tighter than
    the method; an emulation without the lo halves does not (the bound can tell a lost half)."""
    for c, mode in DEVICE:
        if mode != 'bound' and c.N * c.GH * c.GW <= 2500:
            build(c, mode)
    done = 0
    for c in CASES:
        if c.N * c.GH * c.GW > 600 or c.Co * c.Ci > 192 * 64:
            continue
        b = build(c, 'bound')
        rep = (3 * 2.0 ** -22 if c.split == 2 else 2 * 2.0 ** -11) * b.S
        err = (emulate(c, b) - b.ref).abs()
        assert bool((err <= rep).all()), f'{c.id}: emulated split {float((err / rep).max()):.3f} x the representation part'
        if c.split == 2:
            half = types.SimpleNamespace(**{**vars(c), 'split': 1})
            assert bool(((emulate(half, b) - b.ref).abs() > bound_of(c, b, want_of(c)[0])).any()), c.id
        done += 1
    assert done >= 20


# ----------------------------------------------------------------------------------------------------- device helpers
def launch(c, b, ops, gw, ws):
    from rick_amd._lib import lib
    s_co, s_ci, s_t = b.strides
    if c.pk:
        return lib.rick_conv_wgrad_split_f32(p(ops.x), p(ops.xh), p(ops.gy), p(ops.gh), p(gw), s_co, s_ci, s_t, ctypes.byref(b.g),
                                             c.acc, p(ws), stream())
    return lib.rick_conv_wgrad_f32(p(ops.x), p(ops.gy), p(gw), s_co, s_ci, s_t, p(ops.asc), p(ops.bsc), ctypes.byref(b.g), c.acc,
                                   p(ws), stream())


def upload(c, b):
    ops = types.SimpleNamespace(asc=fenced(b.asc), bsc=fenced(b.bsc), xh=None, gh=None)
    ops.gy, ops.gh = split_image(b.gy) if c.pk & 1 else (fenced(b.gy), None)
    ops.x, ops.xh = split_image(b.x) if c.pk & 2 else (fenced(b.x), None)
    return ops


def check_result(c, mode, b, r, got):
    got = got.detach().cpu()
    named = torch.zeros(b.span, dtype=torch.bool)
    named[b.idx] = True
    rest_ok = torch.equal(got[~named].view(torch.int32), b.before[~named].view(torch.int32))
    assert rest_ok, f'{c.id}: {int((got[~named] != b.before[~named]).sum())} elements the launch does not name were changed'
    dev = got[b.idx].reshape(b.ref.shape)
    if mode != 'bound':
        exp = b.ref.float()
        bad = dev != exp
        if bool(bad.any()):
            at = bad.nonzero()
            d = (dev.double() - b.ref)[bad].abs() / b.unit
            raise AssertionError(f'{c.id}: {int(bad.sum())} of {bad.numel()} elements differ (co {sorted(set(at[:, 0].tolist()))[:8]}.., ci '
                                 f'{sorted(set(at[:, 1].tolist()))[:8]}.., taps {sorted(set(at[:, 2].tolist()))}), by {float(d.min())} .. '
                                 f'{float(d.max())} units; first at {tuple(at[0].tolist())}: {float(dev[bad][0])} != {float(exp[bad][0])}')
    else:
        err = (dev.double() - b.ref).abs()
        bnd = bound_of(c, b, r)
        worst = float((err / bnd.clamp_min(1e-300)).max())
        print(f'{c.id}: max |err| / bound = {worst:.4f} (n = {b.n}, nsplit = {r.nsplit})')
        assert bool((err <= bnd).all()), f'{c.id}: |err| up to {worst:.3f} x the a-priori bound'


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@params(DEVICE)
def test_wgrad_forms(c, mode):
    r, want = want_of(c)
    assert want == c.want and r.rc == 0
    b = build(c, mode)
    sat0 = sat_count()
    ops = upload(c, b)
    runs = []
    for _ in range(2 if mode == 'bound' else 1):
        gw, ws = Guarded(b.span, b.before), Guarded(r.ws_floats)
        rc = launch(c, b, ops, gw, ws)
        torch.cuda.synchronize()
        assert rc == 0, f'{c.id}: rc = {rc}'
        gw.assert_bands(c.id + ' gw')
        ws.assert_bands(c.id + ' workspace')
        runs.append(gw)
    check_result(c, mode, b, r, runs[0].v)
    if len(runs) == 2:
        assert torch.equal(runs[0].v.view(torch.int32), runs[1].v.view(torch.int32)), f'{c.id}: two launches differ'
    assert sat_count() == sat0


@gpu
@pytest.mark.parametrize('c', GATES, ids=[c.id for c in GATES])
def test_wgrad_refuses_what_it_has_no_kernel_for(c):
    """RICK_EINVAL before anything is launched: output and workspace keep every sentinel."""
    r, want = want_of(c)
    assert want == c.want and r.rc == EINVAL
    b = types.SimpleNamespace(g=make_geom(c), strides=strides_of(c, make_geom(c)))
    g = b.g
    ops = types.SimpleNamespace(gy=Fenced(g.N * g.OH * g.OW * g.Co), x=Fenced(g.N * g.IH * g.IW * g.Ci), asc=None, bsc=None,
                                gh=Fenced(4) if c.pk & 1 else None, xh=Fenced(4) if c.pk & 2 else None)
    gw, ws = Guarded(g.Co * g.Ci * g.nslices + 64), Guarded(max(r.ws_floats, 4))
    assert launch(c, b, ops, gw, ws) == EINVAL
    torch.cuda.synchronize()
    assert gw.untouched() and ws.untouched()


@gpu
def test_wgrad_refuses_bad_pointers_and_headerless_split_calls():
    """A good geometry (the first case: it runs in test_wgrad_forms), refused for its pointers alone: an operand or a scale table
    4 bytes off the 16-byte alignment, a NULL workspace, rick_conv_wgrad_split_f32 with neither header."""
    from rick_amd._lib import lib
    c = next(k for k in CASES if k.pk == 0 and k.split == 2 and want_of(k)[0].fast)
    r, _ = want_of(c)
    b = build(c, 'exact11')
    s_co, s_ci, s_t = b.strides
    good = types.SimpleNamespace(gy=fenced(b.gy), x=fenced(b.x), asc=fenced(scales('a', (c.N, c.Co), 'exact11')),
                                 bsc=fenced(scales('b', (c.N, c.Ci), 'exact11')))
    gw, ws = Guarded(b.span), Guarded(r.ws_floats)
    gp = ctypes.byref(b.g)
    for name in ('gy', 'x', 'asc', 'bsc'):
        o = types.SimpleNamespace(**vars(good))
        src = getattr(good, name).v
        setattr(o, name, Fenced(src.numel(), src, off=1))
        assert lib.rick_conv_wgrad_f32(p(o.x), p(o.gy), p(gw), s_co, s_ci, s_t, p(o.asc), p(o.bsc), gp, 0, p(ws), stream()) == EINVAL, name
    assert lib.rick_conv_wgrad_f32(p(good.x), p(good.gy), p(gw), s_co, s_ci, s_t, None, None, gp, 0, None, stream()) == EINVAL
    assert lib.rick_conv_wgrad_split_supported(gp) == 1
    assert lib.rick_conv_wgrad_split_f32(p(good.x), None, p(good.gy), None, p(gw), s_co, s_ci, s_t, gp, 0, p(ws), stream()) == EINVAL
    torch.cuda.synchronize()
    assert gw.untouched() and ws.untouched()
