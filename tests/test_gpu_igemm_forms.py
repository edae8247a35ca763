"""Every dispatch form of the forward / data-gradient implicit GEMM (rick_amd/csrc/conv.hip), through the C ABI
(rick_conv_pack_weight, rick_conv_igemm_f32, rick_conv_igemm_act_f32, rick_conv_igemm_split_f32, rick_conv_igemm_multi_f32)
with a hand-built ConvGeom, against the fp64 expression of include/rick_hip.h written out here:

    out[n, gy*os+oy0, gx*os+ox0, co] = tail( alpha * oscale[n,co] * sum_t sum_ci W[wt[t]][co][ci] * (iscale[n,ci] * x[n, gy*is+dy[t], gx*is+dx[t], ci]) )
    tail(v) = gain * lrelu_slope(v + bias[co] + noise_w * noise[n or 0][oy][ox])   (only with an epilogue; act = 0: neither slope nor gain)

with x = 0 outside IH x IW.  The op/ layer is not used.

The launcher is replayed on the host (make_tiling, igemm_tile_positions, igemm_plan_split, the three LDS budgets, igemm_w8_plan
and igemm_s2w8_plan under the rick_conv_tuning values the case sets, the u9 / u9s2 predicates and the branch order of
launch_igemm, the order of igemm_run — eight-wave stride 1, eight-wave stride 2, four-wave —, the block-order branch at the top
of igemm_body, the vec choice of launch_splitk_reduce, plan_multi and its `!m.deep || ngeom == 1` fallback); every case states
the form it reaches as a literal (`want`), which is also its id:

    k<s2,vec,NJ4,NT9,WDMA3,pk0>/nw4/s16x4/red<vec4,noamax>/pos-fastest
    kernel instantiation <SPLIT, VEC, [DEEP,] NJ, NT, WDMA, PKX> / waves / splits x chunks per split / second stage / block order

and the host-only test holds the literal to the replay and the replay to the library (rick_conv_igemm_workspace_bytes,
rick_conv_igemm_multi_workspace_bytes, rick_conv_igemm_split_supported on every geometry of the tables under default and forced
tuning).

Checks, none with a measured tolerance:

  exact11  x, W, bias and noise non-zero integers |v| <= amp <= 4 of mixed sign, iscale / oscale / split_scale in {0.5, 1, 2},
           alpha = 0.25, noise_w = 0.5, slope = 0.25, gain = 2, the weight scale of the packer 1, and sum |terms| < 2**24 units
           for every output element (asserted on the CPU, from an upper bound that needs no contraction).  Every operand fits
           fp16's 11 bits after the power-of-two exponents (per block, per pack, per image), so `lo` is zero, every product,
           every partial sum in any order and every step of the tail is an exact fp32 number, through split-K and both second
           stages: torch.equal to the fp64 result cast to fp32.  Pins indexing, halos, masks, tails, tap-to-slice mapping.
  exact22x / exact22w  (split == 2) one operand (x / W) takes fine() values — 12 significant bits, the last one set, so
           hi != v and lo != 0 — the other small integers.  hi*hi + lo*hi is exact in units of 2**-10, lo*lo is identically
           zero: torch.equal again.  A form that drops or misplaces the `lo` half of either operand — the packed weight's lo
           tile, the lo half of a split image — fails here and nowhere in exact11.  The budget allows K = Ci * ntaps of about
           2 000 at integer amplitude 2 and 4 000 at 1.
  bound    standard-normal operands (one case with per-channel octaves 2**randint(-6, 3) on x), scales in [0.5, 1.5], weight
           scale 2**-0.5; per output element |dev - ref64| <= gain (with act) * the sum of (bound_of):
             3 * 2**-22 * S                     representation: |v - hi - lo| <= 2**-22 |v| on either operand (conv_common.h) and
                                                the dropped lo*lo  (split == 1: 2 * 2**-11 * S);  S = sum |terms|
             2**-27 * (Xmax sum|w| + Wmax sum|x|)   values below the exponent window: 2**-27 of the operand maximum each, times
                                                the other operand (block / pack / image maxima are no larger than the tensor's)
             (K + nsplit + R) * 2**-24 * (S + |bias| + |noise_w * noise|)
                                                fp32 accumulation in any order, K = Ci * ntaps terms, nsplit partial sums and
                                                R = 12 further roundings: the weight-scale product of the packer (1), the
                                                iscale product (1), two more additions per term (three MFMA products), alpha
                                                and oscale (3: s * alpha, oscale * alpha or s * oscale, the product), the tail
                                                (5: + bias, noise_w * noise, + noise, * slope, * gain)
             2**-23 |ref|                       one ulp of the result
           A bound case is launched twice: bit-identical (fixed summation order, no atomics on values).
           The accumulation part grows with K while a lost `lo` half costs about 2**-12 S / sqrt(K): the bound stops seeing a
           lost half at K of a few hundred.  The host-only test shows on the CPU that it sees one on every case with K <= 160
           and prints, by name (LO_BLIND), how far it is from seeing one (0.003 ... 0.016 of the bound) on the forms whose only
           geometries lie beyond the exact22 budget: the split-K nine-tap loops (K = 18 432) and <2,vec,NJ4,NT9,WDMA0>
           (K = 64 512).  The former are the kernel instantiations the 264- and
           272-block cases run under exact22 with one split; for the latter no smaller geometry exists (below), so its `lo` path
           — the commit_patch and weight copy it shares, as source, with every other four-wave form — has no case of its own.

Every device case: output, workspace, amax word, split_out and its header between sentinel bands; output elements the launch
does not name (the other parity classes under os = 2, everything when the call is refused) keep the sentinel bit for bit;
x, iscale, oscale, bias, noise, noise_w, split_scale, the weight, the packed weight and the split-image header are views into
buffers that hold NaN on either side (fp16 NaN halves around a split image); the saturation counter stays put.  epi.amax: the
maximum over the 16 slots equals max |out| of the device output exactly.  epi.split_out: the header is
{2^e, 2^-e, coef * bound, 0} with coef * bound * 2^e in [2**13, 2**14); the decoded image equals fp32(out * split_scale)
exactly in the exact modes and within 2**-22 relative in `bound`, and image and header are bit-equal to rick_split_pack_f32 of
the device output under the same bound.  splitk_fused = 1 cases: three launches on the self-resetting tickets, bit-equal to
the second-stage kernel.  Eight-wave forms on split images: bit-equal to the four-wave form of the same case (one split each).

Forms no geometry under the size cap reaches (production build; no case): <2,vec,NJ2,NT9,WDMA0> and the RICK_WDMA /
RICK_U9_* / RICK_IGEMM_NOUNROLL / RICK_CONV_DEBUG arms exist in the experiment build only.  <2,vec,NJ4,NT9,WDMA0> needs
lds + 16 KB > 80 KB at NPP <= 192, that is nbe * cps >= 57; with one image per tile that is 58 chunks per block without
split-K, out of reach, but five images per 4 x 4 tile reach it at cps = 14 (Ci = 7 168, 16 splits): it has a case.
rick_convt2_f32 (convt2.hip) has its own plan and position map: tests/test_gpu_convt2_forms.py holds its forms to the same checks.
"""
import contextlib
import ctypes
import functools
import math
import types

import pytest
import torch

from rick_amd.synth import synth_tensor
from tests.forms_common import (AMAX_FLOATS, AMAX_STRIDE, DEV, SENT, Fenced, Guarded, _gen, amax_word_check, bound_terms, cdiv,
                                decode_image, f32, fenced, fine, ilog2_ceil, ints, nan_fence_ok, p, rep_of, sat_count, scales, split_halves, split_image,
                                stream)

gpu = pytest.mark.gpu
EINVAL = 22
LDS_MAX = 160 * 1024
WSTEP = 16384
R_ROUND = 12                  # further roundings on a term (module docstring)
TUNE_KEYS = {'igemm_w8': 0, 'igemm_w8_minblk': 1, 'splitk_fused': 2, 'igemm_s2w8': 4}
TUNE_DEFAULT = {'igemm_w8': 0, 'igemm_w8_minblk': 192, 'splitk_fused': 0, 'igemm_s2w8': 2}
TUNES = {'': {}, 'w8': {'igemm_w8': 2, 'igemm_w8_minblk': 1}, 's2w8': {'igemm_s2w8': 2, 'igemm_w8_minblk': 1}, 'no-s2w8': {'igemm_s2w8': 0},
         'fused': {'splitk_fused': 1}}
FORCED = {'igemm_w8': 2, 'igemm_s2w8': 2, 'igemm_w8_minblk': 1}


def tune_of(name):
    return {**TUNE_DEFAULT, **TUNES[name]}


@contextlib.contextmanager
def conv_tuning(kv):
    """rick_conv_tuning for the duration of a block: which kernel FORM a launch takes, never its values."""
    from rick_amd._lib import lib
    prev = {k: lib.rick_conv_tuning(TUNE_KEYS[k], v) for k, v in kv.items()}
    try:
        yield
    finally:
        for k, v in prev.items():
            lib.rick_conv_tuning(TUNE_KEYS[k], v)


def case(**kw):
    return types.SimpleNamespace(**kw)


# ---------------------------------------------------------------------------------------------------------- geometries
def _sq(k, off):
    return [(ky - off, kx - off, ky * k + kx) for ky in range(k) for kx in range(k)]


def _tclasses(k):
    """The output-parity classes of a k x k stride-2 transposed convolution, padding 1: out[2 g + p] takes the kernel rows ky
    with (p + 1 - ky) even from input row g + (p + 1 - ky) / 2."""
    one = lambda par: [((par + 1 - kk) // 2, kk) for kk in range(k) if (par + 1 - kk) % 2 == 0]
    return [(py, px, [(dy, dx, ky * k + kx) for dy, ky in one(py) for dx, kx in one(px)]) for py in (0, 1) for px in (0, 1)]


# kind -> (input stride, output stride, input extent of a grid extent, slices, [(oy0, ox0, taps (dy, dx, slice))])
KINDS = {
    'k3': (1, 1, lambda n: n, 9, [(0, 0, _sq(3, 1))]),                                  # 3 x 3, stride 1, pad 1: negative dy / dx
    'k1': (1, 1, lambda n: n, 1, [(0, 0, [(0, 0, 0)])]),
    'k2': (1, 1, lambda n: n + 1, 4, [(0, 0, _sq(2, 0))]),                              # 2 x 2, pad 0
    'k3s2': (2, 1, lambda n: 2 * n + 1, 9, [(0, 0, _sq(3, 0))]),                        # 3 x 3, stride 2, pad 0
    'k1s2': (2, 1, lambda n: 2 * n - 1, 1, [(0, 0, [(0, 0, 0)])]),
    'c4of9': (1, 1, lambda n: n, 9, [(0, 0, [(-1, -1, 0), (-1, 1, 2), (1, -1, 6), (1, 1, 8)])]),    # a tap subset, nslices = 9
    'k3t': (1, 2, lambda n: n, 9, _tclasses(3)),                                        # classes of 1, 2, 2 and 4 taps
    'k4t': (1, 2, lambda n: n, 16, _tclasses(4)),                                       # four classes of 4 taps
    'k1s4': (4, 1, lambda n: 4 * n - 3, 1, [(0, 0, [(0, 0, 0)])]),                      # 1 x 1, stride 4: the patch outgrows LDS
    'wide': (1, 1, lambda n: n + 1023, 2, [(0, 0, [(0, 0, 0), (0, 1023, 1)])]),         # two taps 1 023 columns apart: PW > 1 023
}


def make_geoms(c, alpha=0.25):
    """The ConvGeom of every class the call names (c.cls: one class of the kind only)."""
    from rick_amd._lib import ConvGeom
    is_, os_, ext, nsl, classes = KINDS[c.kind]
    out = []
    for oy0, ox0, taps in (classes if c.cls is None else [classes[c.cls]]):
        g = ConvGeom()
        g.N, g.IH, g.IW, g.Ci = c.N, ext(c.GH), ext(c.GW), c.Ci
        g.OH, g.OW, g.Co, g.GH, g.GW = c.GH * os_, c.GW * os_, c.Co, c.GH, c.GW
        g.is_, g.os, g.oy0, g.ox0 = is_, os_, oy0, ox0
        g.ntaps, g.nslices = len(taps), nsl
        for t, (dy, dx, wt) in enumerate(taps):
            g.dy[t], g.dx[t], g.wt[t] = dy, dx, wt
        g.split, g.alpha = c.split, alpha
        out.append(g)
    if c.bad == 'ci-unequal':
        out[1].Ci += 32
    return out


def macs_of(c):
    return sum(g.N * g.GH * g.GW * g.Ci * g.Co * g.ntaps for g in make_geoms(c))


# ------------------------------------------------------------------------------------------ host-side launcher replay
def tile_positions(g):
    return 64 if g.is_ >= 2 and g.ntaps > 1 else 128


def make_tiling(g, tile):
    """conv_tiling.h make_tiling."""
    tl = ilog2_ceil(tile)
    tw = min(max(min(ilog2_ceil(g.GW), 4), 2), tl)
    th = min(ilog2_ceil(g.GH), tl - tw)
    t = types.SimpleNamespace(tw=tw, th=th, nb=tile >> (tw + th))
    t.nbe = min(t.nb, g.N)
    t.ntx, t.nty, t.ntn = cdiv(g.GW, 1 << tw), cdiv(g.GH, 1 << th), cdiv(g.N, t.nbe)
    dys, dxs = [g.dy[i] for i in range(g.ntaps)], [g.dx[i] for i in range(g.ntaps)]
    t.PH = ((1 << th) - 1) * g.is_ + (max(dys) - min(dys)) + 1
    t.PW = ((1 << tw) - 1) * g.is_ + (max(dxs) - min(dxs)) + 1
    t.NPP = t.nbe * t.PH * t.PW
    t.nchunks, t.ncot = cdiv(g.Ci, 32), cdiv(g.Co, 128)
    t.nsplit, t.cps = 1, t.nchunks
    t.npos = t.ntx * t.nty * t.ntn
    return t


def plan_split(t, ntaps):
    """igemm_plan_split: minimise waves x (k-steps per block + 32) (+ 6 for a second stage) over up to 16 splits."""
    base = t.npos * t.ncot
    if t.nchunks < 2:
        return
    best_cps, best_cost = t.nchunks, 1 << 30
    for s in range(1, min(t.nchunks, 16) + 1):
        cps = cdiv(t.nchunks, s)
        se = cdiv(t.nchunks, cps)
        cost = cdiv(base * se, 512) * (cps * ntaps + 32) + (6 if se > 1 else 0)
        if cost < best_cost:
            best_cost, best_cps = cost, cps
    t.cps, t.nsplit = best_cps, cdiv(t.nchunks, best_cps)


def _lds_tables(t):
    return ((t.NPP + 3) & ~3) * 4 + t.nbe * t.cps * 32 * 4 + 64


def lds_bytes(t):
    return 2 * WSTEP + 2 * (t.NPP + 1) * 64 + _lds_tables(t)


def w8_lds_bytes(t):
    return 4 * WSTEP + 4 * (t.NPP + 1) * 64 + _lds_tables(t)


def s2w8_lds_bytes(t):
    return 4 * WSTEP + 2 * (t.NPP + 1) * 64 + _lds_tables(t)


def w8_plan(g, tune, pkx):
    w8 = tune['igemm_w8']
    if w8 == 1 and (pkx or g.Ci < 16 * 32):
        return None
    if not w8 or g.split != 2 or g.ntaps != 9 or g.is_ != 1 or g.Ci & 3 or g.GH < 16 or g.GW < 16:
        return None
    t = make_tiling(g, 256)
    if t.nb != 1 or t.NPP > 64 * 6 or t.nchunks < 4 or t.npos * t.ncot < tune['igemm_w8_minblk']:
        return None
    if g.N * g.IH * g.IW * g.Ci * 4 >= (1 << 32) - 256:
        return None
    return t if w8_lds_bytes(t) <= LDS_MAX and t.PH <= 1023 and t.PW <= 1023 else None


def s2w8_plan(g, tune):
    mode = tune['igemm_s2w8']
    if not mode or g.split != 2 or g.ntaps != 9 or g.is_ != 2 or g.Ci & 3 or g.Co & 255 or g.GH < 8 or g.GW < 16:
        return None
    t = make_tiling(g, 128)
    if t.nb != 1 or t.NPP > 64 * 9 or t.nchunks < (8 if mode == 1 else 4):
        return None
    t.ncot = g.Co // 256
    if t.npos * t.ncot < tune['igemm_w8_minblk'] or g.N * g.IH * g.IW * g.Ci * 4 >= (1 << 32) - 256:
        return None
    return t if s2w8_lds_bytes(t) <= LDS_MAX and t.PH <= 1023 and t.PW <= 1023 else None


def kform(S, V, deep, NJ, NT, WDMA, pk, nw=4):
    return f'k<s{S},{"vec" if V else "novec"},{"deep," if deep else ""}NJ{NJ},NT{NT},WDMA{WDMA},pk{int(pk)}>/nw{nw}'


def four_wave_form(g, t, pkx):
    """launch_igemm<SPLIT, VEC>: the instantiation, or None where a split image has no form."""
    S, V, tp = g.split, g.Ci % 4 == 0, tile_positions(g)
    fullk = t.nsplit == 1 or t.cps >= 4
    nine = S == 2 and V and g.ntaps == 9 and fullk and t.cps >= 4
    u9, u9s2 = nine and tp == 128 and t.NPP <= 192, nine and tp == 64 and t.NPP <= 320
    wdma3 = u9 and lds_bytes(t) + WSTEP <= 80 * 1024
    if pkx:
        if u9s2:
            return kform(2, True, False, 2, 9, 2, True)
        if tp == 64:
            return kform(2, True, False, 2, 0, 0, True) if t.NPP <= 320 else None
        if wdma3:
            return kform(2, True, False, 4, 9, 3, True)
        return kform(2, True, True, 4, 0, 0, True) if t.NPP <= 192 else None
    if u9s2:
        return kform(2, True, False, 2, 9, 2, False)
    if tp == 64:
        return kform(S, V, False, 2, 0, 0, False)
    if u9:
        return kform(2, True, False, 4, 9, 3 if wdma3 else 0, False)
    return kform(S, V, t.NPP <= 192, 4, 0, 0, False)


def replay(g, tune, pkx=False, tail='', amax=False, so='', bad=''):
    """igemm_run for one geometry: rc and the gate's name, or the form: kernel / plan / second stage / block order."""
    r = types.SimpleNamespace(rc=0, why=None, form=None, nsplit=1, ws_floats=0, w8=False)

    def refuse(why):
        r.rc, r.why = EINVAL, why
        return r
    t4 = make_tiling(g, tile_positions(g))
    plan_split(t4, g.ntaps)
    r.ws_floats = t4.nsplit * g.N * g.GH * g.GW * g.Co if t4.nsplit > 1 else 0       # rick_conv_igemm_workspace_bytes: the four-wave plan's
    if pkx and (bad == 'hdr-null' or g.Ci & 31 or g.split != 2):
        return refuse('split_f32')
    if bad in ('noise-now', 'noise-nb'):
        return refuse('noise')
    if tail and g.Co & 3:
        return refuse('tail-co4')
    if bad == 'align-bias':
        return refuse('align')
    if so and (g.Co & 3 or bad in ('so-nohdr', 'so-nobound', 'so-coef0')):
        return refuse('split_out-fields')
    if bad.startswith('align-'):               # (split_out / split_scale: the same statement as the split_out fields in the source)
        return refuse('align')
    t = w8_plan(g, tune, pkx)
    if t is not None:
        r.t, r.w8 = t, True
        r.form = kform(2, True, False, 4, 9, 4, pkx, 8) + f'/s1x{t.cps}/nored/pos-fastest'
        return r
    t = s2w8_plan(g, tune)
    if t is not None:
        r.t, r.w8 = t, True
        r.form = kform(2, True, False, 4, 9, 5, pkx, 8) + f'/s1x{t.cps}/nored/co-fastest'
        return r
    r.t, r.nsplit = t4, t4.nsplit
    t = t4
    if t.nsplit > 1 and bad in ('ws-null', 'ws-misaligned'):
        return refuse('workspace')
    if t.nsplit > 1 and so:
        return refuse('split_out-splitk')
    if t.PH > 1023 or t.PW > 1023:             # (one condition with the LDS budget in the source: no patch that wide fits LDS)
        return refuse('ph-pw')
    if lds_bytes(t) > LDS_MAX:
        return refuse('lds')
    k = four_wave_form(g, t, pkx)
    if k is None:
        return refuse('split_f32')
    fused = bool(tune['splitk_fused']) and t.nsplit > 1 and g.Co % 4 == 0 and g.Ci % 4 == 0 and r.ws_floats * 4 < 1 << 32
    stage = 'nored' if t.nsplit == 1 else 'fused' if fused else f'red<{"vec4" if g.Co % 4 == 0 else "elem"},{"amax" if amax else "noamax"}>'
    order = 'pos-fastest' if t.nsplit > 1 or g.is_ < 2 else 'co-fastest'
    r.form = f'{k}/s{t.nsplit}x{t.cps}/{stage}/{order}'
    return r


def replay_multi(gs, tune, bad=''):
    """rick_conv_igemm_multi_f32: plan_multi (128-position tiles, class workspaces rounded to 64 floats), one launch of
    conv_igemm_multi_kernel<SPLIT, VEC> when every class has NPP <= 192 and there is more than one, else a launch per class."""
    r = types.SimpleNamespace(rc=0, why=None, form=None, ws_off=[], ws_floats=0, nsplit=1, w8=False)
    if len(gs) < 1 or len(gs) > 8 or any(g.Ci != gs[0].Ci or g.Co != gs[0].Co or g.split != gs[0].split for g in gs):
        r.rc, r.why = EINVAL, 'multi'
        return r
    if bad.startswith('align-'):
        r.rc, r.why = EINVAL, 'align'
        return r
    ts, deep = [], True
    for g in gs:
        t = make_tiling(g, 128)
        plan_split(t, g.ntaps)
        if lds_bytes(t) > LDS_MAX or t.PH > 1023 or t.PW > 1023:
            r.rc, r.why = EINVAL, 'lds'
            return r
        deep = deep and t.NPP <= 192
        r.ws_off.append(r.ws_floats)
        if t.nsplit > 1:
            r.ws_floats += (t.nsplit * g.N * g.GH * g.GW * g.Co + 63) & ~63
        ts.append(t)
    r.ts, r.nsplit = ts, max(t.nsplit for t in ts)
    plans = '+'.join(f's{t.nsplit}x{t.cps}' for t in ts)
    if r.ws_floats and bad in ('ws-null', 'ws-misaligned'):
        r.rc, r.why = EINVAL, 'workspace'
    elif not deep or len(gs) == 1:
        subs = [replay(g, tune) for g in gs]
        assert all(s.rc == 0 and s.nsplit == t.nsplit for s, t in zip(subs, ts))
        r.form = 'percls[' + '|'.join(s.form for s in subs) + ']'
    else:
        V, red = gs[0].Ci % 4 == 0, f'red<{"vec4" if gs[0].Co % 4 == 0 else "elem"},noamax>'
        r.form = f'multi<s{gs[0].split},{"vec" if V else "novec"}>/c{len(gs)}/{plans}/{red if r.nsplit > 1 else "nored"}'
    return r


def split_supported(g, tune):
    """What rick_conv_igemm_split_supported must say: the replayed rick_conv_igemm_split_f32 finds a form."""
    r = replay(g, tune, pkx=True)
    return int(r.rc == 0)


def want_of(c, tune=None):
    gs = make_geoms(c)
    tune = tune_of(c.tune) if tune is None else tune
    if c.multi:
        if c.bad == 'ngeom0':
            gs = []
        elif c.bad == 'ngeom9':
            gs = gs * 3
        r = replay_multi(gs[:9], tune, c.bad)
    else:
        r = replay(gs[0], tune, bool(c.pk), c.tail, c.amax, c.so, c.bad)
    return r, (r.form if r.rc == 0 else f'EINVAL:{r.why}')


# ------------------------------------------------------------------------------------------------------- case table
def C(kind, N, GH, GW, Ci, Co, want, split=2, isc=0, osc=0, tail='', amax=0, so='', pk=0, tune='', e22=False, amp=4, octaves=0, cls=None,
      multi=0, bad='', also=''):
    """One case; `want` is the literal it must reach.  isc / osc: iscale / oscale given; tail: letters of b(ias), n(oise, one map),
    N (noise, a map per image), a(ct); amax: epi.amax; so: 'o' epi.split_out, 'os' with split_scale; pk: x is a split image;
    tune: a key of TUNES; e22: runs exact22 too; amp: integer amplitude; octaves: per-channel octaves on x in `bound`; cls: one
    parity class of the kind through the single-geometry entry points; multi: rick_conv_igemm_multi_f32; bad: what makes the
    call invalid (refusals); also: a second tuning ('w8', or 'default') under which the same case must give the same bits."""
    tag = f'{kind}-N{N}-{GH}x{GW}-Ci{Ci}-Co{Co}' + (f'-split{split}' if split != 2 else '') + ('-isc' if isc else '') + \
          ('-osc' if osc else '') + (f'-tail:{tail}' if tail else '') + ('-amax' if amax else '') + (f'-so:{so}' if so else '') + \
          ('-pk' if pk else '') + (f'-tune:{tune}' if tune else '') + ('-oct' if octaves else '') + (f'-cls{cls}' if cls is not None else '') + \
          ('-multi' if multi else '') + (f'-bad:{bad}' if bad else '') + (f'-also:{also}' if also else '')
    return case(id=want + '-' + tag, want=want, kind=kind, N=N, GH=GH, GW=GW, Ci=Ci, Co=Co, split=split, isc=isc, osc=osc, tail=tail,
                amax=amax, so=so, pk=pk, tune=tune, e22=e22, amp=amp, octaves=octaves, cls=cls, multi=multi, bad=bad, also=also)


K = kform
CASES = [
    # the simplest forms first: one tile, one split, guarded scalar loads, two-ahead prefetch
    C('k3', 1, 4, 4, 6, 10, K(2, 0, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', e22=True),
    C('k3', 1, 4, 4, 6, 10, K(1, 0, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', split=1, isc=1, osc=1),
    C('k3', 3, 4, 4, 32, 12, K(2, 1, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', e22=True, isc=1, osc=1),
    C('k3', 1, 8, 8, 32, 128, K(1, 1, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', split=1, osc=1),
    # ... masked image slots (N % nbe != 0, nbe > 1), ragged tiles with two images, one live quad in the last chunk
    C('k3', 9, 4, 4, 36, 132, K(2, 1, 0, 4, 0, 0, 0) + '/s2x1/red<vec4,noamax>/pos-fastest', e22=True, isc=1),
    C('k3', 2, 9, 18, 32, 16, K(2, 1, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest'),
    C('k1', 2, 9, 18, 64, 130, K(2, 1, 1, 4, 0, 0, 0) + '/s1x2/nored/pos-fastest', e22=True, isc=1, osc=1),
    C('k2', 2, 8, 8, 64, 16, K(2, 1, 1, 4, 0, 0, 0) + '/s1x2/nored/pos-fastest'),
    C('c4of9', 2, 8, 8, 32, 16, K(2, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', osc=1),
    # the non-DEEP 128-position form: patches above 192 pixels; above 320 the synchronous remaining-items loop
    C('k3', 2, 5, 5, 48, 10, K(2, 1, 0, 4, 0, 0, 0) + '/s2x1/red<elem,noamax>/pos-fastest', e22=True, osc=1),
    C('k3', 2, 5, 5, 6, 10, K(2, 0, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', isc=1, e22=True),
    C('k3', 2, 5, 5, 32, 12, K(1, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', split=1),
    C('k3', 2, 5, 5, 6, 10, K(1, 0, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', split=1),
    C('k1s2', 2, 5, 5, 32, 10, K(2, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/co-fastest', e22=True),
    C('k1s2', 2, 5, 5, 32, 10, K(2, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/co-fastest', isc=1, osc=1),
    # the 64-position stride-2 forms, generic tap loop; NPP = 324: the remaining-items loop
    C('k3s2', 1, 4, 4, 32, 10, K(2, 1, 0, 2, 0, 0, 0) + '/s1x1/nored/co-fastest'),
    C('k3s2', 5, 4, 4, 32, 10, K(2, 1, 0, 2, 0, 0, 0) + '/s1x1/nored/co-fastest', e22=True),
    C('k3s2', 5, 4, 4, 32, 10, K(2, 1, 0, 2, 0, 0, 0) + '/s1x1/nored/co-fastest', isc=1, osc=1),
    C('k3s2', 2, 5, 9, 6, 10, K(2, 0, 0, 2, 0, 0, 0) + '/s1x1/nored/co-fastest', isc=1, e22=True),
    C('k3s2', 1, 4, 4, 36, 260, K(1, 1, 0, 2, 0, 0, 0) + '/s2x1/red<vec4,noamax>/pos-fastest', split=1, osc=1),
    C('k3s2', 2, 5, 9, 6, 10, K(1, 0, 0, 2, 0, 0, 0) + '/s1x1/nored/co-fastest', split=1),
    C('k3s2', 2, 8, 8, 64, 256, K(2, 1, 0, 2, 0, 0, 0) + '/s2x1/red<vec4,noamax>/pos-fastest'),
    # split images on the generic loops
    C('k3', 1, 8, 8, 64, 128, K(2, 1, 1, 4, 0, 0, 1) + '/s2x1/red<vec4,noamax>/pos-fastest', pk=1, e22=True, osc=1),
    C('k1', 3, 8, 8, 32, 20, K(2, 1, 1, 4, 0, 0, 1) + '/s1x1/nored/pos-fastest', pk=1),
    C('k3s2', 2, 5, 9, 64, 128, K(2, 1, 0, 2, 0, 0, 1) + '/s2x1/red<vec4,noamax>/pos-fastest', pk=1, e22=True),
    C('k3s2', 3, 4, 4, 32, 12, K(2, 1, 0, 2, 0, 0, 1) + '/s1x1/nored/co-fastest', pk=1, e22=True, osc=1),
    # the tail, amax and split_out on the direct store
    C('k3', 1, 8, 8, 32, 16, K(2, 1, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', tail='b'),
    C('k3', 1, 8, 8, 32, 16, K(2, 1, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', tail='bna', osc=1, amax=1),
    C('k3', 2, 8, 8, 32, 16, K(2, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', tail='Na', isc=1),
    C('k3', 2, 8, 8, 32, 16, K(2, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', tail='a', isc=1, osc=1),
    C('k3', 2, 8, 8, 32, 10, K(2, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', amax=1, osc=1),
    C('k3', 2, 8, 8, 32, 16, K(2, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', so='o', tail='ba'),
    C('k3', 2, 8, 8, 32, 132, K(2, 1, 0, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', so='os', osc=1, amax=1),
    C('k3s2', 3, 4, 4, 32, 12, K(2, 1, 0, 2, 0, 0, 1) + '/s1x1/nored/co-fastest', pk=1, so='os', tail='bNa'),
    # ... and through the second stage: the four reduce forms, the tail, a short last split
    C('k3', 2, 8, 8, 64, 16, K(2, 1, 0, 4, 0, 0, 0) + '/s2x1/red<vec4,amax>/pos-fastest', amax=1, tail='bna', isc=1, osc=1),
    C('k3', 2, 8, 8, 64, 16, K(2, 1, 0, 4, 0, 0, 0) + '/s2x1/red<vec4,noamax>/pos-fastest', tail='bNa', osc=1),
    C('k3', 2, 8, 8, 64, 10, K(2, 1, 0, 4, 0, 0, 0) + '/s2x1/red<elem,amax>/pos-fastest', amax=1, osc=1),
    C('k3', 2, 8, 8, 64, 10, K(2, 1, 0, 4, 0, 0, 0) + '/s2x1/red<elem,noamax>/pos-fastest'),
    C('c4of9', 26, 9, 17, 160, 128, K(2, 1, 1, 4, 0, 0, 0) + '/s3x2/red<vec4,noamax>/pos-fastest', e22=True, osc=1),
    # the in-launch fix-up
    C('k3', 2, 8, 8, 64, 16, K(2, 1, 0, 4, 0, 0, 0) + '/s2x1/fused/pos-fastest', tune='fused', amax=1, tail='bna', isc=1, osc=1, also='default'),
    C('k3s2', 2, 8, 8, 64, 256, K(2, 1, 0, 2, 0, 0, 0) + '/s2x1/fused/pos-fastest', tune='fused', osc=1, also='default'),
    C('c4of9', 26, 9, 17, 160, 128, K(2, 1, 1, 4, 0, 0, 0) + '/s3x2/fused/pos-fastest', tune='fused', also='default'),
    # one parity class under os = 2 through the single-geometry entry points: the other classes keep the sentinel
    C('k3t', 2, 8, 8, 32, 16, K(2, 1, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest', cls=3, tail='bNa', osc=1),
    C('k4t', 2, 8, 8, 128, 16, K(2, 1, 1, 4, 0, 0, 0) + '/s4x1/red<vec4,amax>/pos-fastest', cls=1, tail='bna', amax=1),
    # the straight-line nine-tap loops under split-K: >= 64 channel chunks (exact11 and bound only: K = 18 432)
    C('k3', 1, 8, 8, 2048, 128, K(2, 1, 0, 4, 9, 3, 0) + '/s16x4/red<vec4,noamax>/pos-fastest', isc=1, osc=1),
    C('k3s2', 1, 8, 8, 2048, 128, K(2, 1, 0, 2, 9, 2, 0) + '/s16x4/red<vec4,noamax>/pos-fastest', osc=1, tail='ba'),
    C('k3', 1, 8, 8, 2048, 128, K(2, 1, 0, 4, 9, 3, 1) + '/s16x4/red<vec4,noamax>/pos-fastest', pk=1),
    C('k3s2', 1, 8, 8, 2048, 128, K(2, 1, 0, 2, 9, 2, 1) + '/s16x4/red<vec4,amax>/pos-fastest', pk=1, amax=1),
    C('k3', 5, 4, 4, 7168, 128, K(2, 1, 0, 4, 9, 0, 0) + '/s16x14/red<vec4,noamax>/pos-fastest', amp=2, isc=1),
    # ... and with one split: >= 257 blocks.  fp32 operands, split images, and the eight-wave forms on the same bits
    C('k3', 43, 17, 17, 128, 128, K(2, 1, 0, 4, 9, 3, 0) + '/s1x4/nored/pos-fastest', e22=True, amp=2),
    C('k3', 43, 17, 17, 128, 128, K(2, 1, 0, 4, 9, 3, 1) + '/s1x4/nored/pos-fastest', pk=1, e22=True, amp=2, also='w8'),
    C('k3s2', 48, 9, 17, 128, 256, K(2, 1, 0, 4, 9, 5, 0, 8) + '/s1x4/nored/co-fastest', e22=True, amp=2),
    C('k3s2', 48, 9, 17, 128, 256, K(2, 1, 0, 2, 9, 2, 0) + '/s1x4/nored/co-fastest', tune='no-s2w8', e22=True, amp=2),
    C('k3s2', 48, 9, 17, 128, 256, K(2, 1, 0, 2, 9, 2, 1) + '/s1x4/nored/co-fastest', tune='no-s2w8', pk=1, e22=True, amp=2, also='default'),
    # the eight-wave forms, forced onto small geometries
    C('k3', 1, 16, 16, 128, 128, K(2, 1, 0, 4, 9, 4, 0, 8) + '/s1x4/nored/pos-fastest', tune='w8', e22=True, amp=2),
    C('k3', 2, 17, 20, 132, 136, K(2, 1, 0, 4, 9, 4, 0, 8) + '/s1x5/nored/pos-fastest', tune='w8', isc=1, osc=1, tail='bna', amax=1, octaves=1),
    C('k3', 2, 17, 20, 128, 132, K(2, 1, 0, 4, 9, 4, 1, 8) + '/s1x4/nored/pos-fastest', tune='w8', pk=1, e22=True, amp=2, so='os'),
    C('k3s2', 1, 8, 16, 128, 256, K(2, 1, 0, 4, 9, 5, 0, 8) + '/s1x4/nored/co-fastest', tune='s2w8', e22=True, amp=2),
    C('k3s2', 2, 9, 17, 132, 256, K(2, 1, 0, 4, 9, 5, 0, 8) + '/s1x5/nored/co-fastest', tune='s2w8', isc=1, osc=1, tail='bNa', amax=1),
    C('k3s2', 2, 9, 17, 128, 512, K(2, 1, 0, 4, 9, 5, 1, 8) + '/s1x4/nored/co-fastest', tune='s2w8', pk=1, e22=True, amp=1, osc=1),
    # the parity classes of transposed convolutions through multi: one launch, and a launch per class (NPP = 200)
    C('k3t', 2, 8, 8, 32, 16, 'multi<s2,vec>/c4/s1x1+s1x1+s1x1+s1x1/nored', multi=1, e22=True, isc=1, osc=1, amp=1),
    C('k4t', 2, 8, 8, 128, 10, 'multi<s2,vec>/c4/s4x1+s4x1+s4x1+s4x1/red<elem,noamax>', multi=1, e22=True, osc=1),
    C('k3t', 1, 8, 8, 128, 16, 'multi<s2,vec>/c4/s1x4+s1x4+s1x4+s4x1/red<vec4,noamax>', multi=1, isc=1),
    C('k3t', 2, 5, 7, 6, 10, 'multi<s2,novec>/c4/s1x1+s1x1+s1x1+s1x1/nored', multi=1, e22=True, isc=1),
    C('k3t', 2, 8, 8, 32, 16, 'multi<s1,vec>/c4/s1x1+s1x1+s1x1+s1x1/nored', multi=1, split=1, osc=1),
    C('k4t', 2, 5, 7, 6, 10, 'multi<s1,novec>/c4/s1x1+s1x1+s1x1+s1x1/nored', multi=1, split=1),
    C('k4t', 8, 4, 4, 128, 16, 'percls[' + '|'.join([K(2, 1, 0, 4, 0, 0, 0) + '/s4x1/red<vec4,noamax>/pos-fastest'] * 4) + ']', multi=1, e22=True, isc=1, osc=1, amp=1),
    C('k3t', 2, 8, 8, 32, 16, 'percls[' + K(2, 1, 1, 4, 0, 0, 0) + '/s1x1/nored/pos-fastest]', multi=1, cls=2),
]
# refused before anything is launched: output and workspace keep every sentinel
GATES = [
    C('k1s4', 1, 8, 16, 32, 16, 'EINVAL:lds'),
    C('wide', 1, 1, 1, 4, 16, 'EINVAL:ph-pw'),
    C('k3', 2, 8, 8, 64, 16, 'EINVAL:workspace', bad='ws-null'),
    C('k3', 2, 8, 8, 64, 16, 'EINVAL:workspace', bad='ws-misaligned'),
    C('k4t', 2, 8, 8, 128, 16, 'EINVAL:workspace', multi=1, bad='ws-null'),
    C('k3', 2, 8, 8, 64, 16, 'EINVAL:split_out-splitk', so='o'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:split_out-fields', so='o', bad='so-nohdr'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:split_out-fields', so='o', bad='so-nobound'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:split_out-fields', so='o', bad='so-coef0'),
    C('k3', 2, 8, 8, 32, 10, 'EINVAL:split_out-fields', so='o'),
    C('k3', 2, 8, 8, 32, 10, 'EINVAL:tail-co4', tail='b'),
    C('k3', 2, 8, 8, 32, 10, 'EINVAL:tail-co4', tail='a'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:noise', tail='n', bad='noise-now'),
    C('k3', 3, 8, 8, 32, 16, 'EINVAL:noise', tail='N', bad='noise-nb'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-x'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-out'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-w'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-isc', isc=1),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-osc', osc=1),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-bias', tail='b'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-so', so='o'),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-ss', so='os'),
    C('k3t', 2, 8, 8, 32, 16, 'EINVAL:align', bad='align-x', multi=1),
    C('k3', 2, 8, 8, 48, 16, 'EINVAL:split_f32', pk=1),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:split_f32', pk=1, split=1),
    C('k3', 2, 8, 8, 32, 16, 'EINVAL:split_f32', pk=1, bad='hdr-null'),
    C('k3', 2, 5, 5, 32, 16, 'EINVAL:split_f32', pk=1),                 # NPP = 200 > 192 at stride 1
    C('k3s2', 5, 4, 4, 32, 16, 'EINVAL:split_f32', pk=1),               # NPP = 324 > 320 at stride 2
    C('k3t', 2, 8, 8, 32, 16, 'EINVAL:multi', multi=1, bad='ngeom0'),
    C('k3t', 2, 8, 8, 32, 16, 'EINVAL:multi', multi=1, bad='ngeom9'),
    C('k3t', 2, 8, 8, 32, 16, 'EINVAL:multi', multi=1, bad='ci-unequal'),
]
REQUIRED_GATES = {'lds', 'ph-pw', 'workspace', 'split_out-splitk', 'split_out-fields', 'tail-co4', 'noise', 'align', 'split_f32', 'multi'}
# forms whose geometries all lie beyond the exact22 budget, where the bound cannot see a lost `lo` half (module docstring)
LO_BLIND = {K(2, 1, 0, 4, 9, 3, 0) + '/s16x4', K(2, 1, 0, 2, 9, 2, 0) + '/s16x4', K(2, 1, 0, 4, 9, 3, 1) + '/s16x4', K(2, 1, 0, 2, 9, 2, 1) + '/s16x4',
            K(2, 1, 0, 4, 9, 0, 0) + '/s16x14'}


def modes_of(c):
    return ('exact11', 'bound') + (('exact22x', 'exact22w') if c.e22 else ())


DEVICE = [(c, m) for c in CASES for m in modes_of(c)]


def params(pairs):
    return pytest.mark.parametrize('c,mode', pairs, ids=[f'{c.id}-{m}' for c, m in pairs])


# ----------------------------------------------------------------------------------------------------------- inputs
def shifted(g, B, dy, dx):
    """B [N, IH, IW, Ci] -> [N, GH, GW, Ci]: B[n, gy*is + dy, gx*is + dx], zero outside the input."""
    IH, IW = B.shape[1], B.shape[2]
    iy, ix = torch.arange(g.GH) * g.is_ + dy, torch.arange(g.GW) * g.is_ + dx
    ok = ((iy >= 0) & (iy < IH))[:, None] & ((ix >= 0) & (ix < IW))[None, :]
    return B[:, iy.clamp(0, IH - 1)][:, :, ix.clamp(0, IW - 1)] * ok[None, :, :, None].to(B.dtype)


def contract(g, X, Wm):
    """sum_t sum_ci Wm[co, ci, wt[t]] * X[n, gy*is+dy[t], gx*is+dx[t], ci] -> [N, GH, GW, Co] (fp64)."""
    acc = torch.zeros(g.N * g.GH * g.GW, g.Co, dtype=torch.float64)
    for t in range(g.ntaps):
        acc += shifted(g, X, g.dy[t], g.dx[t]).reshape(-1, g.Ci) @ Wm[:, :, g.wt[t]].t()
    return acc.reshape(g.N, g.GH, g.GW, g.Co)


def taps_sum(g, X):
    """sum_t sum_ci X[n, gy*is+dy[t], gx*is+dx[t], ci] -> [N, GH, GW]."""
    return sum(shifted(g, X, g.dy[t], g.dx[t]).sum(-1) for t in range(g.ntaps))


def _key(c, mode):
    return (c.kind, c.N, c.GH, c.GW, c.Ci, c.Co, c.split, c.isc, c.osc, c.tail, c.so, c.amp, c.octaves, c.cls, bool(c.multi), mode)


@functools.lru_cache(maxsize=2)
def _inputs(key):
    kind, N, GH, GW, Ci, Co, split, isc, osc, tail, so, amp, octaves, cls, multi, mode = key
    c = case(kind=kind, N=N, GH=GH, GW=GW, Ci=Ci, Co=Co, split=split, cls=cls, bad='')
    sid = f'igf/{kind}/{N}/{GH}x{GW}/{Ci}/{Co}/{mode}'
    exact = mode != 'bound'
    gs = make_geoms(c, 0.25 if exact else f32(1 / math.sqrt(2)))
    g0 = gs[0]
    b = types.SimpleNamespace(gs=gs, alpha=g0.alpha, exact=exact, wscale=1.0 if exact else f32(2 ** -0.5), K=max(g.ntaps for g in gs) * Ci)
    xs, ws = (N, g0.IH, g0.IW, Ci), (Co, Ci, g0.nslices)
    if mode == 'bound':
        b.x, b.w = synth_tensor(sid + '/x', xs), synth_tensor(sid + '/w', ws)
        if octaves:
            b.x = b.x * torch.exp2(torch.randint(-6, 4, (N, 1, 1, Ci), generator=_gen(sid + '/oct')).float())
    elif mode == 'exact11':
        b.x, b.w = ints(sid + '/x', xs, amp), ints(sid + '/w', ws, amp)
    elif mode == 'exact22x':
        b.x, b.w = fine(sid + '/x', xs), ints(sid + '/w', ws, min(amp, 2))
    else:
        b.x, b.w = ints(sid + '/x', xs, min(amp, 2)), fine(sid + '/w', ws)
    b.isc = scales(sid + '/isc', (N, Ci), mode) if isc else None
    b.osc = scales(sid + '/osc', (N, Co), mode) if osc else None
    b.ss = scales(sid + '/ss', (N, Co), mode) if 's' in so else None
    OH, OW = g0.OH, g0.OW
    b.bias = (ints(sid + '/bias', (Co,), 4) if exact else synth_tensor(sid + '/bias', (Co,))) if 'b' in tail else None
    nb = N if 'N' in tail else 1
    b.noise = (ints(sid + '/noise', (nb, OH, OW), 4) if exact else synth_tensor(sid + '/noise', (nb, OH, OW))) if tail.lower().count('n') else None
    b.nw = (0.5 if exact else f32(0.3)) if b.noise is not None else 0.0
    b.act, b.slope, b.gain = int('a' in tail), (0.25 if exact else f32(0.2)), (2.0 if exact else f32(math.sqrt(2)))
    # the premises of the exact modes, from an upper bound of sum |terms| that needs no contraction
    b.X = b.x.double() * (b.isc.double()[:, None, None, :] if isc else 1.0)
    b.W = b.w.double() * float(b.wscale)
    b.unit = b.alpha * (0.5 if isc else 1.0) * (0.5 if osc else 1.0) * (1.0 if mode in ('exact11', 'bound') else 2.0 ** -10)
    if exact:
        omax = float(b.osc.max()) if osc else 1.0
        sub = max(float(taps_sum(g, b.X.abs()).max()) for g in gs) * float(b.W.abs().max()) * b.alpha * omax
        sub += (4.0 if b.bias is not None else 0.0) + (0.5 * 4.0 if b.noise is not None else 0.0)
        assert sub / b.unit < 2 ** 24, f'{sid}: sum |terms| <= {sub / b.unit} units: not exact in fp32'
        for name, v in (('x', b.X), ('w', b.W)):
            lim = 11 if mode == 'exact11' or name != mode[-1] else 12
            q = v.abs()
            assert bool((q * 2.0 ** 11 == (q * 2.0 ** 11).round()).all()) and float(q.max()) / float(q[q > 0].min()) <= 16, name
            assert lim == 12 or bool((q.float().half().double() == q).all()), f'{name}: more than 11 bits'
    for name, v, Cn in (('x', b.x, Ci), ('w', b.w.permute(0, 2, 1), Ci), ('w', b.w.permute(1, 2, 0), Co)):
        assert float(v.min()) < 0 < float(v.max()), f'{name}: one sign only'
        if v.numel() // Cn <= 1 << 16:
            assert torch.unique(v.reshape(-1, Cn).t(), dim=0).shape[0] == Cn, f'{name}: two equal channels'
    assert N == 1 or torch.unique(b.x.reshape(N, -1), dim=0).shape[0] == N, 'x: two equal images'
    return b


def inputs(c, mode):
    return _inputs(_key(c, mode))


@functools.lru_cache(maxsize=2)
def _reference(key):
    """The fp64 result on the whole output [N, OH, OW, Co] with the mask of named positions, and the sums the bound needs."""
    b = _inputs(key)
    mode = key[-1]
    g0 = b.gs[0]
    N, OH, OW, Co = g0.N, g0.OH, g0.OW, g0.Co
    r = types.SimpleNamespace(ref=torch.zeros(N, OH, OW, Co, dtype=torch.float64), named=torch.zeros(N, OH, OW, Co, dtype=torch.bool))
    r.bnd, r.per_split = torch.zeros_like(r.ref), torch.zeros_like(r.ref)
    osc = b.osc.double()[:, None, None, :] if b.osc is not None else 1.0
    for g in b.gs:
        sl = (slice(None), slice(g.oy0, None, g.os), slice(g.ox0, None, g.os))
        v = b.alpha * osc * contract(g, b.X, b.W)
        add = torch.zeros(N, g.GH, g.GW, 1, dtype=torch.float64)
        if b.bias is not None:
            v = v + b.bias.double()
            add = add + b.bias.double().abs()
        if b.noise is not None:
            nz = float(b.nw) * b.noise.double()[sl][..., None]
            v, add = v + nz, add + nz.abs()
        if b.act:
            v = torch.where(v > 0, v, v * float(b.slope)) * float(b.gain)
        r.ref[sl], r.named[sl] = v, True
        if mode == 'bound':
            S = b.alpha * (osc if b.osc is None else osc.abs()) * contract(g, b.X.abs(), b.W.abs())
            sw = torch.stack([b.W.abs()[:, :, g.wt[t]].sum(1) for t in range(g.ntaps)]).sum(0)            # [Co]
            wn = b.alpha * (osc if b.osc is None else osc.abs()) * (float(b.X.abs().max()) * sw + float(b.W.abs().max()) * taps_sum(g, b.X.abs())[..., None])
            rep = rep_of(g.split)
            r.rep = rep
            gain = float(b.gain) if b.act else 1.0
            r.bnd[sl] = bound_terms(S, wn, add, g.Ci * g.ntaps, R_ROUND, rep) * gain
            t4 = make_tiling(g, tile_positions(g))
            plan_split(t4, g.ntaps)
            r.per_split[sl] = (t4.nsplit if t4.nsplit > 1 else 0) * 2.0 ** -24 * (S + add) * gain        # (not on the eight-wave forms: one split)
            r.S = S                                 # (of the last class: the emulation test runs single-class cases)
    if b.exact:
        assert torch.equal(r.ref.float().double(), r.ref) and not bool((r.ref == SENT).any())
        if b.ss is not None:
            assert float((r.ref * b.ss.double()[:, None, None, :]).abs().max()) / (b.unit * (0.25 if b.act else 1.0) * 0.5) < 2 ** 22, 'split_out: more than 22 bits'
    assert float(r.ref[r.named].min()) < 0 < float(r.ref[r.named].max())
    return r


def bound_of(r, w8=False):
    return r.bnd + (0.0 if w8 else r.per_split) + 2.0 ** -23 * r.ref.abs()


def emulate(c, b, lo=True):
    """The documented split on the CPU with ONE exponent per operand (maximum placed in [4, 8), as CV_EXP_TARGET = 2):
    hi = fp16(v * 2^e), lo = fp16(v * 2^e - hi), products hi*hi + hi*lo + lo*hi (no lo*lo), summed in fp64; no tail."""
    g = b.gs[0]
    xh, xl, ux = split_halves(b.X, lo and c.split == 2)
    wh, wl, uw = split_halves(b.W, lo and c.split == 2)
    osc = b.osc.double()[:, None, None, :] if b.osc is not None else 1.0
    return b.alpha * osc * ux * uw * (contract(g, xh, wh) + contract(g, xh, wl) + contract(g, xl, wh))


# ---------------------------------------------------------------------------------------------------- host-only tests
def _feat(c, r, gs):
    """The coverage items one case reaches, named from the replay (REQUIRED lists what the tables must reach together)."""
    f = set()
    forms = r.form[7:-1].split('|') if r.form.startswith('percls[') else [r.form]
    for fm in forms:
        if fm.startswith('k<'):
            f.add('/'.join(fm.split('/')[:2]))
            f |= {s for s in fm.split('/')[3:] if s != 'nored'}
    if r.form.startswith('multi<'):
        f |= {r.form.split('/')[0], 'multi one launch'} | {s for s in r.form.split('/')[3:] if s != 'nored'}
        if sum(o > 0 for o in r.ws_off) > 1:
            f.add('multi class workspaces')
    if r.form.startswith('percls[') and len(gs) > 1:
        f.add('multi per class')
    ts = r.ts if c.multi else [r.t]
    for g, t in zip(gs, ts):
        f.add('one split' if t.nsplit == 1 else 'several splits')
        f |= {'short last split' if t.nchunks % t.cps else '', 'nbe>1' if t.nbe > 1 else '', 'N%nbe' if g.N % t.nbe else '',
              'ragged tiles, two images' if (g.GH % (1 << t.th) or g.GW % (1 << t.tw)) and g.N > 1 else '',
              'Co%128' if g.Co % 128 else '', 'Ci%32' if g.Ci % 32 else '', 'Ci%4' if g.Ci % 4 else '',
              'single live quad' if g.Ci % 32 in (1, 2, 3, 4) else '',
              ('Co%4 split-K store' if t.nsplit > 1 else 'Co%4 direct store') if g.Co % 4 else '',
              'negative dy/dx' if min(g.dy[i] for i in range(g.ntaps)) < 0 else '', 'tap subset' if g.ntaps < g.nslices and g.os == 1 else ''}
        if not r.w8 and not c.pk and 'NT0' in r.form and 'deep' not in r.form and t.NPP > 320:
            f.add('sync loop' + ('+iscale' if c.isc else ''))
        if g.os == 2:
            f.add(f'os2:{"k3t" if g.nslices == 9 else "k4t"}:{g.oy0}{g.ox0}')
    f.add(f'epilogue<{int(bool(c.osc))},{int(bool(c.tail))}>')
    f |= {'bias only' if c.tail == 'b' else '', 'noise nb=1' if 'n' in c.tail else '', 'noise nb=N' if 'N' in c.tail else '',
          'act' if 'a' in c.tail else '', 'tail without act' if c.tail and 'a' not in c.tail else '',
          ('amax second stage' if r.nsplit > 1 else 'amax direct') if c.amax else '', 'split_out' if c.so == 'o' else '',
          'split_out+scale' if c.so == 'os' else '', 'w8 == four-wave' if c.also == 'w8' else '', 's2w8 == four-wave' if c.also == 'default' and c.tune == 'no-s2w8' else '',
          's2w8 by default' if r.w8 and c.tune == '' else ''}
    if c.e22:
        f |= {'e22:' + x for x in f if x.startswith('k<') or x.startswith('multi<')}
    f.discard('')
    return f


_SV = [(s, v) for s in (1, 2) for v in (0, 1)]
_KERNELS = ({K(2, 1, 0, 4, 9, w, pk, 8) for w in (4, 5) for pk in (0, 1)}
            | {K(2, 1, 0, 2, 9, 2, 1), K(2, 1, 0, 2, 0, 0, 1), K(2, 1, 0, 4, 9, 3, 1), K(2, 1, 1, 4, 0, 0, 1)}
            | {K(2, 1, 0, 2, 9, 2, 0), K(2, 1, 0, 4, 9, 3, 0), K(2, 1, 0, 4, 9, 0, 0)}
            | {K(s, v, d, nj, 0, 0, 0) for s, v in _SV for d, nj in ((0, 2), (1, 4), (0, 4))})
REQUIRED = (
    _KERNELS | {f'multi<s{s},{"vec" if v else "novec"}>' for s, v in _SV}
    | {f'red<{v},{a}>' for v in ('vec4', 'elem') for a in ('amax', 'noamax')} | {'fused', 'pos-fastest', 'co-fastest'}
    # exact22 on every instantiation that has a geometry inside its budget (LO_BLIND: the others)
    | {'e22:' + k for k in _KERNELS if k != K(2, 1, 0, 4, 9, 0, 0) and not k.startswith('k<s1')} | {'e22:multi<s2,vec>', 'e22:multi<s2,novec>'}
    | {'one split', 'several splits', 'short last split', 'nbe>1', 'N%nbe', 'ragged tiles, two images', 'Co%128', 'Co%4 direct store',
       'Co%4 split-K store', 'Ci%32', 'Ci%4', 'single live quad', 'sync loop', 'sync loop+iscale', 'negative dy/dx', 'tap subset'}
    | {f'epilogue<{o},{e}>' for o in (0, 1) for e in (0, 1)}
    | {'bias only', 'noise nb=1', 'noise nb=N', 'act', 'tail without act', 'amax direct', 'amax second stage', 'split_out', 'split_out+scale'}
    | {f'os2:{k}:{py}{px}' for k in ('k3t', 'k4t') for py in (0, 1) for px in (0, 1)}
    | {'multi one launch', 'multi per class', 'multi class workspaces', 'w8 == four-wave', 's2w8 == four-wave', 's2w8 by default'})


def test_case_ids_replay_and_library_agree():
    """No device.  Every case's literal `want` is what the replayed launcher picks under the case's tuning; the replay's plans are
    the library's own (workspace bytes of one geometry and of a class list) and rick_conv_igemm_split_supported says, for every
    geometry of the tables under default and forced tuning, whether the replayed launcher finds a split-image form; the tables
    reach the whole coverage list and every gate; the size caps hold."""
    from rick_amd._lib import ConvGeom, lib
    assert len({c.id for c in CASES + GATES}) == len(CASES + GATES)
    reached, gates, big = set(), set(), set()
    for c in CASES + GATES:
        gs = make_geoms(c)
        r, want = want_of(c)
        assert want == c.want, f'{c.id}: the replay reaches {want}'
        for g in gs:
            one = replay(g, TUNE_DEFAULT)
            assert lib.rick_conv_igemm_workspace_bytes(ctypes.byref(g)) == one.ws_floats * 4, c.id
            for tune in (TUNE_DEFAULT, {**TUNE_DEFAULT, **FORCED}):
                with conv_tuning(tune):
                    got = lib.rick_conv_igemm_split_supported(ctypes.byref(g))
                assert got == split_supported(g, tune), f'{c.id}: rick_conv_igemm_split_supported says {got} (forced = {tune is not TUNE_DEFAULT})'
        if c.multi and c.bad not in ('ngeom0', 'ngeom9', 'ci-unequal'):
            arr = (ConvGeom * len(gs))(*gs)
            assert lib.rick_conv_igemm_multi_workspace_bytes(arr, len(gs)) == replay_multi(gs, TUNE_DEFAULT).ws_floats * 4, c.id
        if c in CASES:
            assert r.rc == 0 and not c.bad, c.id
            reached |= _feat(c, r, gs)
            assert not c.e22 or c.split == 2
            m = macs_of(c)
            assert m <= 6e9, c.id
            if m > 2e9:
                big.add((c.kind, c.N, c.GH, c.GW, c.Ci, c.Co))
        else:
            assert r.rc == EINVAL, c.id
            gates.add(r.why)
    assert not REQUIRED - reached, f'not reached: {sorted(REQUIRED - reached)}'
    assert not REQUIRED_GATES - gates, f'gates not reached: {sorted(REQUIRED_GATES - gates)}'
    assert len(big) <= 2, big
    assert len(DEVICE) + len(GATES) <= 220
    for k in LO_BLIND:
        assert any(c.want.startswith(k.split('/s')[0]) and '/' + k.split('/')[-1] + '/' in c.want and not c.e22 for c in CASES), k


def test_exact_inputs_fit_and_the_bound_sees_a_lost_lo_half_where_it_can():
    """No device.  Every exact-mode builder passes its own assertions (sum |terms| < 2**24 units from an upper bound, operands of
    11 / 12 bits inside the 32x window, distinct channels and images, mixed signs).  On the single-geometry cases with
    K <= 160 the CPU emulation of the documented split stays inside the representation part of the bound alone (that part is no
    tighter than the method), and an emulation without the lo halves leaves the whole bound: the bound can tell a lost half.
    On the LO_BLIND forms the emulation with both halves is inside the bound too; whether the one without is, is printed."""
    for c, mode in DEVICE:
        if mode != 'bound':
            inputs(c, mode)
    done, blind = 0, 0
    for c in CASES:
        k = c.want.split('/')[0] + '/nw4/' + c.want.split('/')[2] if c.want.startswith('k<') else ''
        small = not c.multi and c.cls is None and c.Ci * len(KINDS[c.kind][4][0][2]) <= 160 and not c.tail
        if not small and k not in LO_BLIND:
            continue
        plain = types.SimpleNamespace(**{**vars(c), 'tail': '', 'so': ''})
        b, r = inputs(plain, 'bound'), _reference(_key(plain, 'bound'))
        err = (emulate(c, b) - r.ref).abs()
        assert bool((err <= r.rep * r.S).all()), f'{c.id}: emulated split {float((err / (r.rep * r.S)).max()):.3f} x the representation part'
        if c.split == 2:
            worst = float(((emulate(c, b, lo=False) - r.ref).abs() / bound_of(r)).max())
            if small:
                assert worst > 1, f'{c.id}: the bound does not see a lost lo half ({worst:.3f})'
                done += 1
            else:
                print(f'{c.id}: without lo {worst:.3f} x the bound (K = {b.K})')
                blind += 1
    assert done >= 8 and blind == len(LO_BLIND)


# ----------------------------------------------------------------------------------------------------- device helpers
def pack_weight(c, b):
    from rick_amd._lib import lib
    g = b.gs[0]
    nbytes = lib.rick_conv_packed_bytes(g.Co, g.Ci, g.nslices)
    src, pk = fenced(b.w), Fenced(nbytes // 4)
    rc = lib.rick_conv_pack_weight(p(src), g.Ci * g.nslices, g.nslices, 1, g.Co, g.Ci, g.nslices, float(b.wscale), g.split,
                                   p(pk), stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert nan_fence_ok(pk), 'rick_conv_pack_weight wrote outside the packed image'
    return pk


def upload(c, b, bad=''):
    """Every operand of the call as a fenced view; `bad` misaligns one."""
    o = types.SimpleNamespace()
    off = lambda name: 1 if bad == 'align-' + name else 0
    o.w = pack_weight(c, b)
    if off('w'):
        o.w = types.SimpleNamespace(v=o.w.buf[65:])
    o.x, o.hdr = split_image(b.X.float()) if c.pk else (fenced(b.x, off('x')), None)
    if bad == 'hdr-null':
        o.hdr = None
    o.isc = None if c.pk else fenced(b.isc, off('isc'))
    o.osc, o.ss = fenced(b.osc, off('osc')), fenced(b.ss, off('ss'))
    o.bias, o.noise = fenced(b.bias, off('bias')), fenced(b.noise)
    o.nw = fenced(torch.tensor([float(b.nw)])) if b.noise is not None and bad != 'noise-now' else None
    return o


def epilogue_of(c, b, o, out, bad=''):
    """-> (ConvEpilogue or None, amax word, split image, header, bound word)."""
    from rick_amd._lib import ConvEpilogue
    if not (c.tail or c.amax or c.so):
        return None, None, None, None, None
    g = b.gs[0]
    e = ConvEpilogue()
    e.bias, e.noise, e.noise_w = p(o.bias), p(o.noise), p(o.nw)
    e.noise_nb = (g.N if 'N' in c.tail else 1) if bad != 'noise-nb' else 2
    e.act, e.slope, e.gain, e.split_coef = b.act, float(b.slope), float(b.gain), 1.0
    word = Guarded(AMAX_FLOATS, torch.zeros(AMAX_FLOATS)) if c.amax else None
    e.amax = p(word)
    img = hdr = bw = None
    if c.so:
        img, hdr = Guarded(out.v.numel()), Guarded(4)
        wd = torch.zeros(AMAX_FLOATS)
        wd[5 * AMAX_STRIDE] = b.so_bound
        bw = fenced(wd)
        e.split_out = img.buf[img.lo + 1:].data_ptr() if bad == 'align-so' else p(img)
        e.split_hdr, e.split_bound = None if bad == 'so-nohdr' else p(hdr), None if bad == 'so-nobound' else p(bw)
        e.split_coef, e.split_scale = 0.0 if bad == 'so-coef0' else 1.5, p(o.ss)
    return e, word, img, hdr, bw


def launch(c, b, o, out, ws, epi, bad=''):
    from rick_amd._lib import ConvGeom, lib
    gs = b.gs
    ep = ctypes.byref(epi) if epi is not None else None
    wsp = None if bad == 'ws-null' else ws.buf[ws.lo + 1:].data_ptr() if bad == 'ws-misaligned' else p(ws)
    outp = out.buf[out.lo + 1:].data_ptr() if bad == 'align-out' else p(out)
    if c.multi:
        n = 0 if bad == 'ngeom0' else 9 if bad == 'ngeom9' else len(gs)
        arr = (ConvGeom * 9)(*(gs * 3)[:9]) if bad == 'ngeom9' else (ConvGeom * len(gs))(*gs)
        return lib.rick_conv_igemm_multi_f32(p(o.x), p(o.w), outp, p(o.isc), p(o.osc), arr, n, wsp, stream())
    if c.pk:
        return lib.rick_conv_igemm_split_f32(p(o.x), p(o.hdr), p(o.w), outp, p(o.osc), ctypes.byref(gs[0]), ep, wsp, stream())
    if epi is None:
        return lib.rick_conv_igemm_f32(p(o.x), p(o.w), outp, p(o.isc), p(o.osc), ctypes.byref(gs[0]), wsp, stream())
    return lib.rick_conv_igemm_act_f32(p(o.x), p(o.w), outp, p(o.isc), p(o.osc), ctypes.byref(gs[0]), ep, wsp, stream())


def run_once(c, b, o, r, tune):
    """One launch under `tune` into fresh guarded buffers -> the buffers, checked for their bands."""
    g0 = b.gs[0]
    out, ws = Guarded(g0.N * g0.OH * g0.OW * g0.Co), Guarded(max(r.ws_floats, 4))
    epi, word, img, hdr, bw = epilogue_of(c, b, o, out)
    with conv_tuning(tune):
        rc = launch(c, b, o, out, ws, epi)
        torch.cuda.synchronize()
    assert rc == 0, f'{c.id}: rc = {rc}'
    for what, gd in (('out', out), ('workspace', ws), ('amax word', word), ('split_out', img), ('split_hdr', hdr)):
        if gd is not None:
            gd.assert_bands(f'{c.id} {what}')
    return types.SimpleNamespace(out=out, ws=ws, word=word, img=img, hdr=hdr, bw=bw)


def check_result(c, mode, b, r, rf, got):
    dev = got.out.v.detach().cpu().reshape(rf.ref.shape)
    keep = dev[~rf.named]
    assert bool((keep.view(torch.int32) == torch.tensor(SENT).view(torch.int32)).all()), \
        f'{c.id}: {int((keep != SENT).sum())} elements the launch does not name were changed'
    if mode != 'bound':
        exp = rf.ref.float()
        bad = (dev != exp) & rf.named
        if bool(bad.any()):
            at = bad.nonzero()
            d = (dev.double() - rf.ref)[bad].abs() / b.unit
            raise AssertionError(f'{c.id}: {int(bad.sum())} of {int(rf.named.sum())} elements differ (n {sorted(set(at[:, 0].tolist()))[:8]}.., rows '
                                 f'{sorted(set(at[:, 1].tolist()))[:8]}.., cols {sorted(set(at[:, 2].tolist()))[:8]}.., co '
                                 f'{sorted(set(at[:, 3].tolist()))[:8]}..), by {float(d.min())} .. {float(d.max())} units; first at '
                                 f'{tuple(at[0].tolist())}: {float(dev[bad][0])} != {float(exp[bad][0])}')
    else:
        err = (dev.double() - rf.ref).abs()[rf.named]
        bnd = bound_of(rf, r.w8)[rf.named]
        worst = float((err / bnd.clamp_min(1e-300)).max())
        print(f'{c.id}: max |err| / bound = {worst:.4f} (K = {b.K}, nsplit = {r.nsplit})')
        assert bool((err <= bnd).all()), f'{c.id}: |err| up to {worst:.3f} x the a-priori bound'
    if c.amax:
        amax_word_check(got.word.v.detach().cpu(), float(dev[rf.named].abs().max()), c.id)
    if c.so:
        from rick_amd._lib import lib
        hdr = got.hdr.v.detach().cpu()
        bound = float(torch.tensor(1.5) * torch.tensor(b.so_bound))
        e = math.log2(float(hdr[0]))
        assert e == int(e) and float(hdr[1]) == 2.0 ** -e and float(hdr[2]) == bound and float(hdr[3]) == 0.0, f'{c.id}: header {hdr.tolist()}'
        assert 2 ** 13 <= bound * 2.0 ** e < 2 ** 14, f'{c.id}: header {hdr.tolist()}'
        scaled = got.out.v.reshape(rf.ref.shape) * (o_ss(b) if b.ss is not None else 1.0)
        dec = decode_image(got.img.v.detach().cpu(), hdr).reshape(rf.ref.shape)
        if mode != 'bound':
            assert torch.equal(dec, scaled.cpu()), f'{c.id}: the split image is not fp32(out * split_scale)'
        else:
            assert bool(((dec.double() - scaled.cpu().double()).abs() <= 2.0 ** -22 * scaled.cpu().double().abs() + 2.0 ** -25 * 2.0 ** -e).all()), c.id
        src, img2, hdr2 = fenced(scaled), Fenced(scaled.numel(), image=True), Fenced(4)
        g0 = b.gs[0]
        assert lib.rick_split_pack_f32(p(src), p(img2), p(hdr2), p(got.bw), None, 1.5, g0.N * g0.OH * g0.OW, g0.Co, stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(img2.v.view(torch.int32), got.img.v.view(torch.int32)) and torch.equal(hdr2.v.view(torch.int32), got.hdr.v.view(torch.int32)), \
            f'{c.id}: not the image rick_split_pack_f32 makes of the output'


def o_ss(b):
    return b.ss.to(DEV)[:, None, None, :]


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@params(DEVICE)
def test_igemm_forms(c, mode):
    r, want = want_of(c)
    assert want == c.want and r.rc == 0
    b, rf = inputs(c, mode), _reference(_key(c, mode))
    if c.so:
        ss = b.ss.double()[:, None, None, :] if b.ss is not None else 1.0
        b.so_bound = f32(float((rf.ref * ss).abs().max()) * (1.0 if b.exact else 1.01) / 1.5 * 1.25)
    sat0 = sat_count()
    o = upload(c, b)
    tune = tune_of(c.tune)
    runs = [run_once(c, b, o, r, tune) for _ in range(3 if c.tune == 'fused' else 2 if mode == 'bound' else 1)]
    check_result(c, mode, b, r, rf, runs[0])
    same = lambda a, bb: torch.equal(a.out.v.view(torch.int32), bb.out.v.view(torch.int32)) and \
        (a.word is None or torch.equal(a.word.v[::AMAX_STRIDE].max().view(torch.int32), bb.word.v[::AMAX_STRIDE].max().view(torch.int32)))
    for other in runs[1:]:
        assert same(runs[0], other), f'{c.id}: two launches differ'
    if c.also:
        alt = {'default': '', 'w8': 'w8'}[c.also]
        r2, want2 = want_of(types.SimpleNamespace(**{**vars(c), 'tune': alt}))
        assert r2.rc == 0 and want2 != want and (c.tune == 'fused' or r2.w8), f'{c.id}: the twin reaches {want2}'
        assert same(runs[0], run_once(c, b, o, r2, tune_of(alt))), f'{c.id}: not the bits of {want2}'
    assert nan_fence_ok(o.w), f'{c.id}: the packed weight was written'
    assert sat_count() == sat0


@gpu
@pytest.mark.parametrize('c', GATES, ids=[c.id for c in GATES])
def test_igemm_refuses_what_it_has_no_kernel_for(c):
    """RICK_EINVAL before anything is launched: output, workspace, amax word and split image keep every sentinel."""
    r, want = want_of(c)
    assert want == c.want and r.rc == EINVAL
    b = types.SimpleNamespace(**{**vars(inputs(c, 'exact11')), 'gs': make_geoms(c), 'so_bound': 1.0})
    o = upload(c, b, c.bad)
    g0 = b.gs[0]
    out, ws = Guarded(g0.N * g0.OH * g0.OW * g0.Co + 4), Guarded(max(r.ws_floats, 4) + 4)
    epi, word, img, hdr, _ = epilogue_of(c, b, o, out, c.bad)
    assert launch(c, b, o, out, ws, epi, c.bad) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched() and ws.untouched() and (img is None or (img.untouched() and hdr.untouched()))
    if c.pk and c.bad != 'hdr-null' and c.split == 2 and c.Ci % 32 == 0:
        from rick_amd._lib import lib
        assert lib.rick_conv_igemm_split_supported(ctypes.byref(g0)) == 0
