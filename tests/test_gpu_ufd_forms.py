"""Every dispatch form of the FIR family (rick_amd/csrc/upfirdn2d.hip: the 4x4 up-1 kernel in its 12 instantiations, the generic
channels-last kernel with and without the extended result handling, the planar kernel; rick_amd/csrc/generic.hip: the fp64 /
fp16 kernel), through the C ABI (rick_upfirdn2d_f32, rick_upfirdn2d_act_f32, rick_upfirdn2d_ex_f32, rick_upfirdn2d_any,
rick_upfirdn2d_plan, rick_upfirdn2d_adjoint_rows), against the fp64 reference of tests/ufd_f64.py, which is written from the
operator's definition (zero-stuff, pad / crop, correlate with the flipped taps, decimate) and held here to the committed
reference-derived goldens and to the scalar C oracle.  The method is that of tests/test_gpu_convt2_forms.py;
tests/forms_common.py holds what the files share.

The planner is replayed on the host (plan_replay: the 4x4 gate, the two tile-shrinking loops with their 60 KB / 64 KB limits,
grids, the planar slab loop, every refusal); every case states the form it reaches as a literal (`want`), which is also its id:

    k4<d1,8x8,cb16,tail,xo>/g6x2x3     instantiation <DOWN, tile, float4 per pixel, TAIL, XO> / grid (tiles x slabs x images)
    nhwc<xo>/cb16/t2x4/in14x16/lds57920/g2x1x1
    planar/t16x64/in19x67/g1x6/L1      L: launches (the slab loop)
    EINVAL:<gate>

The host-only test holds the literal to the replay and the replay to rick_upfirdn2d_plan (all 12 fields) on every case and on a
seeded sweep of 4 000 geometries under both values of RICK_TUNE_UFD_TILE16, rick_upfirdn2d_adjoint_rows to both, and asserts on
the sweep that the staged window covers every input row and column the tile's outputs touch: output o of an axis reads the
canvas positions o * down ... o * down + k - 1; canvas position q holds input sample i iff q - pad0 == i * up; the window starts
at the first sample at or after the first output's first position.  None of that uses tile_in_extent.

exact  inputs are non-zero integers |v| <= amp of both signs, taps are the distinct integers +-1 ... +-kh*kw in a seeded order
       (no tap pattern is its own x-flip, y-flip or transpose: asserted), bias / noise / noise strength / the prefilled output of
       `accumulate` are integers, slope, gain and chan_scale powers of two; amp * sum |taps| + tail + accumulate < 2**24 units
       (asserted), so every partial sum in any order is an fp32 number: torch.equal to the fp64 result.  The tolerance is zero.
order  standard-normal inputs and taps (plain launches): bit-equal to oracle.c_ref.upfirdn2d_c, the y-outer / x-inner fmaf order
       that all three kernels document.

Refusals (RICK_EINVAL on the host, every buffer keeps its sentinels): the table follows the code gate by gate.  "ex on planar" is
refused by rick_upfirdn2d_ex_f32's own minor % 4 check before the planner's gate can see it; only rick_upfirdn2d_plan (has_ex
with minor 1) reaches that gate, in the sweep.  The channels-last kernels make 16-byte accesses: input, out, chan_scale and the
split image off a 16-byte boundary are refused, and no case launches with a misaligned pointer that the library accepts (the
planar kernel's accesses are 4-byte: its cases offset input and output by 1, 2 and 3 floats).  A tail that carries amax or
split_out (fields of the convolution's epilogue) is refused.

Every launch: the output (and amax word, split image, header, partial rows) lies between sentinel bands that stay intact, the
operands are views with NaN on both sides, the result holds no NaN, the saturation count does not move.
"""
import ctypes
import functools
import math
import random
import types

import numpy as np
import pytest
import torch

from rick_amd.synth import synth_tensor
from tests import ufd_f64 as R
from tests.cases import UPFIRDN_CASES, upfirdn_kernel
from tests.forms_common import (AMAX_FLOATS, AMAX_STRIDE, DEV, SENT, Fenced, Guarded, amax_word_check, cdiv, decode_image, fenced, ints,
                                p, sat_count, scales, stream)

gpu = pytest.mark.gpu
EINVAL = 22
K4_T8, K4_T16, K4_D2, NHWC, PLANAR = range(5)          # RICK_UFD_* (include/rick_hip.h)
TUNE_UFD_TILE16 = 3
SLOPE, GAIN, NW = 0.25, 2.0, 3.0                         # tail: powers of two, integer noise strength
ADJ_SLOPE, ADJ_GAIN = 0.5, 2.0


def case(**kw):
    return types.SimpleNamespace(**kw)


class tile16:
    """rick_conv_tuning(RICK_TUNE_UFD_TILE16, on), put back on the way out."""

    def __init__(self, on):
        self.on = int(on)

    def __enter__(self):
        from rick_amd._lib import lib
        self.prev = lib.rick_conv_tuning(TUNE_UFD_TILE16, self.on)

    def __exit__(self, *exc):
        from rick_amd._lib import lib
        lib.rick_conv_tuning(TUNE_UFD_TILE16, self.prev)


# ------------------------------------------------------------------------------------------------ host-side planner replay
def tdiv(a, b):
    """C's integer division (towards zero): what the output-size expression of the library and of the reference extension uses."""
    return abs(a) // b * (1 if a >= 0 else -1)


def out_hw(H, W, kh, kw, up, down, pad):
    return tdiv(H * up[1] + pad[2] + pad[3] - kh, down[1]) + 1, tdiv(W * up[0] + pad[0] + pad[1] - kw, down[0]) + 1


def tile_in_extent(t, down, k, up):
    return ((t - 1) * down + k - 1) // up + 2


def plan_replay(major, H, W, minor, kh, kw, up, down, pad, has_tail, has_ex, aligned16, t16):
    """ufd_plan -> (None, plan) or (the gate's name, None).  up = (x, y), down = (x, y), pad = (x0, x1, y0, y1)."""
    (ux, uy), (dx, dy) = up, down
    if min(major, H, W, minor, kh, kw, ux, uy, dx, dy) <= 0:
        return 'size', None
    oh, ow = out_hw(H, W, kh, kw, up, down, pad)
    if oh <= 0 or ow <= 0:
        return 'empty', None
    P = case(oh=oh, ow=ow, launches=1, gz=1)
    if minor % 64 == 0 and kh == 4 and kw == 4 and ux == 1 and uy == 1 and dx == dy and dx in (1, 2) and major <= 65535 and \
            minor // 64 <= 65535 and aligned16:
        if dx == 1 and t16 and oh >= 32 and ow >= 32:
            if 2 * (minor // 64) > 65535:
                return 'grid', None
            P.kernel, P.toh, P.tow, P.cb4 = K4_T16, 16, 16, 8
        elif dx == 1:
            P.kernel, P.toh, P.tow, P.cb4 = K4_T8, 8, 8, 16
        else:
            P.kernel, P.toh, P.tow, P.cb4 = K4_D2, 4, 8, 16
        P.tih, P.tiw = (P.toh - 1) * dy + 4, (P.tow - 1) * dx + 4
        P.lds = P.tih * P.tiw * P.cb4 * 16
        P.gx, P.gy, P.gz = cdiv(ow, P.tow) * cdiv(oh, P.toh), minor // (P.cb4 * 4), major
        return None, P
    if has_tail:
        return 'tail-off-k4', None
    if minor % 4 == 0:
        cb4 = min(minor, 64) // 4
        if minor % (cb4 * 4):
            return 'minor', None
        if not aligned16:
            return 'align', None
        toh = tow = 8
        while True:
            tih, tiw = tile_in_extent(toh, dy, kh, uy), tile_in_extent(tow, dx, kw, ux)
            lds = ((kh * kw + 3) & ~3) * 4 + tih * tiw * cb4 * 16
            if lds <= 60 * 1024 or (toh == 1 and tow == 1):
                if lds > 64 * 1024:
                    return 'lds', None
                if major > 65535:
                    return 'major', None
                P.kernel, P.toh, P.tow, P.tih, P.tiw, P.cb4, P.lds = NHWC, toh, tow, tih, tiw, cb4, lds
                P.gx, P.gy, P.gz = cdiv(ow, tow) * cdiv(oh, toh), minor // (cb4 * 4), major
                return None, P
            if toh >= tow and toh > 1:
                toh >>= 1
            else:
                tow >>= 1
    if has_ex:
        return 'ex-planar', None
    if minor != 1:
        return 'minor', None
    toh, tow = 16, 64
    while True:
        tih, tiw = tile_in_extent(toh, dy, kh, uy), tile_in_extent(tow, dx, kw, ux)
        lds = (kh * kw + tih * tiw) * 4
        if lds <= 60 * 1024 or (toh == 1 and tow == 1):
            if lds > 64 * 1024:
                return 'lds', None
            P.kernel, P.toh, P.tow, P.tih, P.tiw, P.cb4, P.lds = PLANAR, toh, tow, tih, tiw, 0, lds
            P.gx, P.gy, P.launches = cdiv(ow, tow) * cdiv(oh, toh), min(major, 65535), cdiv(major, 65535)
            return None, P
        if toh >= tow and toh > 1:
            toh >>= 1
        else:
            tow >>= 1


def fields(P):
    return [P.kernel, P.toh, P.tow, P.tih, P.tiw, P.lds, P.gx, P.gy, P.gz, P.launches, P.oh, P.ow]


def lib_plan(major, H, W, minor, kh, kw, up, down, pad, has_tail, has_ex, aligned16):
    from rick_amd._lib import lib
    out = (ctypes.c_int * 12)(*([-1] * 12))
    rc = lib.rick_upfirdn2d_plan(major, H, W, minor, kh, kw, up[0], up[1], down[0], down[1], *pad, int(has_tail), int(has_ex), int(aligned16), out)
    return rc, list(out)


def form_of(P, has_tail, has_ex):
    if P.kernel in (K4_T8, K4_T16, K4_D2):
        return (f'k4<d{2 if P.kernel == K4_D2 else 1},{P.toh}x{P.tow},cb{P.cb4},{"tail" if has_tail else "notail"},{"xo" if has_ex else "noxo"}>'
                f'/g{P.gx}x{P.gy}x{P.gz}')
    if P.kernel == NHWC:
        return f'nhwc<{"xo" if has_ex else "noxo"}>/cb{P.cb4}/t{P.toh}x{P.tow}/in{P.tih}x{P.tiw}/lds{P.lds}/g{P.gx}x{P.gy}x{P.gz}'
    return f'planar/t{P.toh}x{P.tow}/in{P.tih}x{P.tiw}/g{P.gx}x{P.gy}/L{P.launches}'


def ex_flags(c):
    return set(c.ex.split('+')) if c.ex else set()


def replay(c):
    """The entry point's own gates, then upfirdn2d_impl, for one case -> (gate name or None, plan or None)."""
    x, bad = ex_flags(c), c.bad
    (ux, uy), (dx, dy) = c.up, c.down
    has_tail, has_ex = bool(c.tail), c.entry == 'ex' and bad != 'ex-null'
    if c.entry == 'act' and not has_tail:
        return 'tail-null', None
    if c.entry == 'ex':
        if bad == 'ex-null' or c.minor & 3:
            return 'ex-minor', None
        if 'split' in x and (bad in ('split-nohdr', 'split-nobound', 'split-coef', 'split-align') or c.minor & 31):
            return 'split-args', None
        if 'null' in x and not ('nof32' in x and 'acc' not in x):
            return 'out-null', None
        if 'adj' in x and not (c.k == (4, 4) and c.up == (1, 1) and c.down == (1, 1) and c.minor % 64 == 0 and not has_tail
                               and bad not in ('adj-align', 'part-align')):
            return 'adj', None
    if bad in ('null-in', 'null-k', 'null-out') or ('null' in x and 'split' not in x):
        return 'null', None
    if bad in ('tail-amax', 'tail-split'):
        return 'tail-fields', None
    aligned16 = bad not in ('align-in', 'align-out', 'align-cs') and (c.off % 4 == 0)
    why, P = plan_replay(c.major, c.H, c.W, c.minor, *c.k, c.up, c.down, c.pad, has_tail, has_ex, aligned16, c.t16)
    if why:
        return why, None
    if P.kernel != PLANAR and has_tail:
        if bad in ('noise-now', 'noise-nb'):
            return 'tail-noise', None
        if bad == 'bias-align':
            return 'tail-bias', None
    return None, P


def want_of(c):
    why, P = replay(c)
    return P, (f'EINVAL:{why}' if why else form_of(P, bool(c.tail), c.entry == 'ex'))


# ------------------------------------------------------------------------------------------------------- case table
def C(want, entry, major, H, W, minor, k=(4, 4), up=(1, 1), down=(1, 1), pad=(0, 0, 0, 0), tail='', ex='', t16=0, off=0, amp=8, bad=''):
    """One case; `want` is the literal it must reach.  entry: f32 / act / ex.  k = (kh, kw), up = (x, y), down = (x, y), pad = (x0,
    x1, y0, y1).  tail: letters b (bias), n / N (noise with noise_nb 1 / major), a (activation).  ex: '+'-joined flags of
    rick_split_out — acc, nof32, null (out == NULL), amax, split, b1 (bound1), c3 (bound_coef 3, else 0.5), cs (chan_scale), adj,
    part (adj_partials), low (a bound 16x too small).  t16: under RICK_TUNE_UFD_TILE16.  off: input and output offset by `off`
    floats.  bad: what makes the call invalid (refusals)."""
    tag = (f'{entry}-M{major}-{H}x{W}-m{minor}-k{k[0]}x{k[1]}-u{up[0]}{up[1]}-d{down[0]}{down[1]}-p{",".join(map(str, pad))}'
           + (f'-tail:{tail}' if tail else '') + (f'-ex:{ex}' if ex else '') + ('-t16' if t16 else '') + (f'-off{off}' if off else '')
           + (f'-bad:{bad}' if bad else ''))
    return case(id=want + '-' + tag, tag=tag, want=want, entry=entry, major=major, H=H, W=W, minor=minor, k=k, up=up, down=down, pad=pad,
                tail=tail, ex=ex, t16=t16, off=off, amp=amp, bad=bad)


P4 = (2, 1, 0, 3)             # four different pads
CASES = [
    # ---- 4x4 up-1 path: (DOWN, tile, CB4) x TAIL x XO
    C('k4<d1,8x8,cb16,notail,noxo>/g6x1x3', 'f32', 3, 18, 11, 64, pad=P4),                       # ragged in both axes, N = 3
    C('k4<d1,8x8,cb16,notail,noxo>/g24x2x1', 'f32', 1, 21, 61, 128, pad=(2, 1, 2, 1)),           # 3 x 8 tiles exactly: re-dealt grid
    C('k4<d1,8x8,cb16,notail,noxo>/g1x1x1', 'f32', 1, 1, 3, 64, pad=(2, 2, 5, 4)),               # in_h = 1, input < tile, pad > 3
    C('k4<d1,8x8,cb16,notail,noxo>/g2x1x3', 'f32', 3, 14, 24, 64, pad=(-2, -3, -1, -2)),         # negative pads
    C('k4<d1,8x8,cb16,tail,noxo>/g6x2x3', 'act', 3, 18, 11, 128, pad=P4, tail='bNa'),
    C('k4<d1,8x8,cb16,tail,noxo>/g4x1x1', 'act', 1, 16, 16, 64, pad=(1, 2, 2, 1), tail='b'),
    C('k4<d1,8x8,cb16,tail,noxo>/g24x1x3', 'act', 3, 61, 21, 64, pad=(1, 2, 1, 2), tail='na'),   # 8 x 3 tiles
    C('k4<d1,8x8,cb16,tail,noxo>/g6x1x3', 'act', 3, 18, 11, 64, pad=P4, tail='N'),
    C('k4<d1,8x8,cb16,notail,xo>/g6x1x3', 'ex', 3, 18, 11, 64, pad=P4, ex='acc+amax'),
    C('k4<d1,8x8,cb16,notail,xo>/g6x2x1', 'ex', 1, 18, 11, 128, pad=P4, ex='nof32+split+cs'),
    C('k4<d1,8x8,cb16,notail,xo>/g4x1x3', 'ex', 3, 13, 13, 64, pad=(2, 1, 2, 1), ex='nof32+null+split+b1+c3'),
    C('k4<d1,8x8,cb16,notail,xo>/g4x1x1', 'ex', 1, 13, 13, 64, pad=(2, 1, 2, 1), ex='split+amax+low'),
    C('k4<d1,8x8,cb16,notail,xo>/g24x1x3', 'ex', 3, 21, 61, 64, pad=(2, 1, 2, 1), ex='nof32+null+split+adj+part'),     # re-dealt grid
    C('k4<d1,8x8,cb16,notail,xo>/g6x1x3', 'ex', 3, 18, 11, 64, pad=P4, ex='adj+part+amax'),                            # ragged, not re-dealt
    C('k4<d1,8x8,cb16,notail,xo>/g16x2x1', 'ex', 1, 29, 29, 128, pad=(2, 1, 2, 1), ex='adj+part+acc'),                 # 4 x 4 tiles, re-dealt
    C('k4<d1,8x8,cb16,tail,xo>/g6x1x3', 'ex', 3, 18, 11, 64, pad=P4, tail='bNa', ex='amax+split+cs+c3'),
    C('k4<d1,8x8,cb16,tail,xo>/g4x2x1', 'ex', 1, 13, 13, 128, pad=(2, 1, 2, 1), tail='bn', ex='acc+split+b1'),
    C('k4<d1,16x16,cb8,notail,noxo>/g9x2x3', 'f32', 3, 38, 40, 64, pad=P4, t16=1),
    C('k4<d1,16x16,cb8,notail,noxo>/g8x4x1', 'f32', 1, 32, 64, 128, pad=(2, 1, 2, 1), t16=1),      # 2 x 4 tiles exactly, re-dealt
    C('k4<d1,16x16,cb8,tail,noxo>/g9x2x3', 'act', 3, 38, 40, 64, pad=P4, tail='bNa', t16=1),
    C('k4<d1,16x16,cb8,notail,xo>/g9x2x3', 'ex', 3, 38, 40, 64, pad=P4, ex='adj+part+nof32+null+split', t16=1),
    C('k4<d1,16x16,cb8,notail,xo>/g8x4x1', 'ex', 1, 32, 64, 128, pad=(2, 1, 2, 1), ex='acc+amax+split+cs', t16=1),
    C('k4<d1,16x16,cb8,tail,xo>/g9x2x3', 'ex', 3, 38, 40, 64, pad=P4, tail='bn', ex='amax+split', t16=1),
    C('k4<d2,4x8,cb16,notail,noxo>/g6x1x3', 'f32', 3, 21, 20, 64, down=(2, 2), pad=P4),
    C('k4<d2,4x8,cb16,notail,noxo>/g8x2x1', 'f32', 1, 15, 63, 128, down=(2, 2), pad=(2, 1, 2, 1)),  # 2 x 4 tiles exactly, re-dealt
    C('k4<d2,4x8,cb16,notail,noxo>/g1x1x1', 'f32', 1, 1, 2, 64, down=(2, 2), pad=(4, 5, 2, 2)),
    C('k4<d2,4x8,cb16,tail,noxo>/g6x1x3', 'act', 3, 21, 20, 64, down=(2, 2), pad=P4, tail='bNa'),
    C('k4<d2,4x8,cb16,notail,xo>/g6x1x3', 'ex', 3, 21, 20, 64, down=(2, 2), pad=P4, ex='nof32+split+b1'),
    C('k4<d2,4x8,cb16,tail,xo>/g6x2x1', 'ex', 1, 21, 20, 128, down=(2, 2), pad=P4, tail='na', ex='acc+amax+split+cs'),
    # ---- generic channels-last: cb4, each way of failing the 4x4 gate, tiles
    C('nhwc<noxo>/cb1/t8x8/in12x12/lds2368/g4x1x2', 'f32', 2, 12, 9, 4, pad=P4),
    C('nhwc<noxo>/cb2/t8x8/in12x11/lds4272/g4x1x3', 'f32', 3, 9, 13, 8, k=(4, 3), pad=P4),
    C('nhwc<noxo>/cb8/t8x8/in12x12/lds18496/g4x1x2', 'f32', 2, 12, 9, 32, pad=P4),                 # minor 32: the gate's minor % 64 alone
    C('nhwc<xo>/cb8/t8x8/in12x12/lds18496/g4x1x2', 'ex', 2, 12, 9, 32, pad=P4, ex='acc+amax+split+cs'),
    C('nhwc<noxo>/cb16/t8x8/in11x11/lds31024/g4x1x2', 'f32', 2, 12, 9, 64, k=(3, 3), pad=(1, 2, 0, 3)),      # kh, kw != 4
    C('nhwc<noxo>/cb16/t8x8/in7x7/lds12608/g6x2x1', 'f32', 1, 11, 7, 128, up=(2, 2), pad=P4),               # up 2
    C('nhwc<xo>/cb16/t8x8/in7x7/lds12608/g6x1x3', 'ex', 3, 11, 7, 64, up=(2, 2), pad=P4, ex='acc+amax'),     # (the adjoint of down 2)
    C('nhwc<noxo>/cb16/t4x4/in14x14/lds50240/g4x1x2', 'f32', 2, 20, 17, 64, down=(3, 3), pad=P4),            # down 3
    C('nhwc<noxo>/cb16/t8x8/in19x12/lds58432/g4x1x2', 'f32', 2, 20, 9, 64, down=(1, 2), pad=P4),             # down_x != down_y
    C('nhwc<xo>/cb16/t8x8/in12x7/lds21568/g4x1x2', 'ex', 2, 12, 7, 64, up=(2, 1), pad=P4, ex='nof32+null+split'),      # up_x != up_y
    C('nhwc<noxo>/cb16/t8x8/in9x12/lds27664/g4x1x2', 'f32', 2, 12, 12, 64, k=(1, 4), pad=(2, 1, 0, 0)),
    C('nhwc<noxo>/cb16/t8x8/in12x9/lds27664/g4x1x2', 'f32', 2, 12, 12, 64, k=(4, 1), pad=(0, 0, 0, 3)),
    C('nhwc<noxo>/cb16/t2x4/in14x16/lds57920/g15x1x2', 'f32', 2, 9, 9, 64, k=(12, 12), pad=(5, 6, 6, 5), amp=4),        # shrunk, non-square
    C('nhwc<xo>/cb16/t1x1/in15x15/lds58384/g6x1x1', 'ex', 1, 3, 4, 64, k=(14, 14), pad=(6, 6, 6, 6), ex='acc+amax', amp=4),
    C('nhwc<noxo>/cb16/t1x1/in15x16/lds62288/g4x1x2', 'f32', 2, 3, 3, 64, k=(14, 15), pad=(6, 7, 6, 6), amp=4),         # 60 KB < LDS <= 64 KB
    # ---- planar
    C('planar/t16x64/in20x68/g4x6/L1', 'f32', 6, 17, 70, 1, pad=P4),
    C('planar/t16x64/in20x68/g1x3/L1', 'f32', 3, 9, 9, 1, pad=(1, 1, 1, 1), off=1),
    C('planar/t16x64/in11x35/g1x3/L1', 'f32', 3, 4, 5, 1, up=(2, 2), pad=(2, 1, 2, 1), off=2),
    C('planar/t16x64/in35x131/g1x2/L1', 'f32', 2, 16, 15, 1, down=(2, 2), pad=(1, 1, 1, 1), off=3),
    C('planar/t8x16/in61x126/g2x2/L1', 'f32', 2, 70, 70, 1, k=(4, 5), down=(8, 8), pad=P4),           # shrunk by a large down
    C('planar/t16x64/in18x66/g1x65535/L2', 'f32', 65538, 2, 2, 1, k=(2, 2), pad=(1, 0, 0, 1)),        # the slab loop
    C('planar/t16x64/in15x39/g2x3/L1', 'f32', 3, 9, 9, 1, k=(12, 12), up=(2, 2), pad=(6, 5, 6, 5), amp=4),             # golden ada_up2_k12
    C('planar/t16x64/in43x139/g1x3/L1', 'f32', 3, 33, 33, 1, k=(12, 12), down=(2, 2), pad=(5, 5, 5, 5), amp=4),        # golden ada_down2_k12
    C('planar/t16x64/in8x24/g1x1/L1', 'f32', 1, 5, 5, 1, k=(6, 6), up=(3, 3), pad=(3, 2, 3, 2)),                     # golden up3_k6
    C('planar/t16x64/in20x68/g1x2/L1', 'f32', 2, 17, 17, 1, pad=(-1, -2, -1, -2)),                                   # golden negpad
    # ---- planar: the remaining geometries of the committed goldens (tests/cases.py), here with asymmetric taps
    C('planar/t16x64/in20x68/g1x2/L1', 'f32', 2, 17, 17, 1, pad=(1, 1, 1, 1)),
    C('planar/t16x64/in20x68/g2x2/L1', 'f32', 2, 16, 16, 1, pad=(2, 2, 2, 2)),
    C('planar/t16x64/in20x68/g1x2/L1', 'f32', 2, 16, 16, 1, pad=(1, 1, 1, 1)),
    C('planar/t16x64/in11x35/g1x2/L1', 'f32', 2, 8, 8, 1, up=(2, 2), pad=(2, 1, 2, 1)),
    C('planar/t16x64/in11x35/g1x2/L1', 'f32', 2, 4, 4, 1, up=(2, 2), pad=(2, 1, 2, 1)),
    C('planar/t16x64/in35x131/g1x2/L1', 'f32', 2, 16, 16, 1, down=(2, 2), pad=(1, 1, 1, 1)),
    C('planar/t16x64/in35x131/g1x1/L1', 'f32', 1, 7, 7, 1, down=(2, 2), pad=(1, 1, 1, 1)),
    C('planar/t16x64/in18x66/g1x2/L1', 'f32', 2, 8, 8, 1, up=(2, 2), down=(2, 2), pad=(1, 1, 1, 1)),
    C('planar/t16x64/in20x68/g1x2/L1', 'f32', 2, 7, 12, 1, pad=(2, 1, 2, 1)),
    C('planar/t16x64/in19x67/g1x2/L1', 'f32', 2, 8, 8, 1, k=(3, 3), pad=(1, 1, 1, 1)),
]
G0 = dict(major=2, H=12, W=9, minor=64)          # the refusals' geometry where none is needed


def G(want, entry='f32', **kw):
    d = dict(G0, pad=(1, 2, 2, 1))
    d.update(kw)
    return C(want, entry, d.pop('major'), d.pop('H'), d.pop('W'), d.pop('minor'), **d)


# refused on the host before anything is launched: the output keeps every sentinel
GATES = [
    G('EINVAL:null', bad='null-in'), G('EINVAL:null', bad='null-k'), G('EINVAL:null', bad='null-out'),
    G('EINVAL:size', major=0), G('EINVAL:size', H=0), G('EINVAL:size', W=-1), G('EINVAL:size', minor=0), G('EINVAL:size', k=(0, 4)),
    G('EINVAL:size', k=(4, 0)), G('EINVAL:size', up=(0, 1)), G('EINVAL:size', up=(1, 0)), G('EINVAL:size', down=(0, 1)),
    G('EINVAL:size', down=(1, -1)),
    G('EINVAL:empty', pad=(-5, -3, 0, 0)), G('EINVAL:empty', pad=(0, 0, -6, -4)),
    G('EINVAL:tail-null', 'act'),
    G('EINVAL:tail-off-k4', 'act', tail='b', k=(3, 3)), G('EINVAL:tail-off-k4', 'act', tail='b', up=(2, 2)),
    G('EINVAL:tail-off-k4', 'act', tail='b', minor=32), G('EINVAL:tail-off-k4', 'act', tail='b', minor=1),
    G('EINVAL:tail-off-k4', 'ex', tail='b', ex='amax', down=(1, 2)),
    G('EINVAL:tail-noise', 'act', tail='n', bad='noise-now'), G('EINVAL:tail-noise', 'act', tail='N', bad='noise-nb'),
    G('EINVAL:tail-bias', 'act', tail='b', bad='bias-align'),
    G('EINVAL:tail-fields', 'act', tail='b', bad='tail-amax'), G('EINVAL:tail-fields', 'ex', tail='b', ex='amax', bad='tail-split'),
    G('EINVAL:ex-minor', 'ex', bad='ex-null'), G('EINVAL:ex-minor', 'ex', ex='amax', minor=6), G('EINVAL:ex-minor', 'ex', ex='amax', minor=1),
    G('EINVAL:split-args', 'ex', ex='split', bad='split-nohdr'), G('EINVAL:split-args', 'ex', ex='split', bad='split-nobound'),
    G('EINVAL:split-args', 'ex', ex='split', minor=16), G('EINVAL:split-args', 'ex', ex='split', bad='split-coef'),
    G('EINVAL:split-args', 'ex', ex='split', bad='split-align'),
    G('EINVAL:out-null', 'ex', ex='null+amax'), G('EINVAL:out-null', 'ex', ex='null+nof32+acc+split'),
    G('EINVAL:adj', 'ex', ex='adj', k=(3, 3)), G('EINVAL:adj', 'ex', ex='adj', up=(2, 2)), G('EINVAL:adj', 'ex', ex='adj', down=(2, 2)),
    G('EINVAL:adj', 'ex', ex='adj', minor=32), G('EINVAL:adj', 'ex', ex='adj', tail='b'),
    G('EINVAL:adj', 'ex', ex='adj', bad='adj-align'), G('EINVAL:adj', 'ex', ex='adj+part', bad='part-align'),
    G('EINVAL:minor', 'ex', ex='amax', minor=72), G('EINVAL:minor', minor=72), G('EINVAL:minor', minor=3), G('EINVAL:minor', minor=6),
    G('EINVAL:major', major=65536, H=1, W=1, minor=4, k=(1, 1), pad=(0, 0, 0, 0)),
    G('EINVAL:lds', k=(16, 16), pad=(8, 8, 8, 8)),
    G('EINVAL:align', k=(3, 3), bad='align-in'), G('EINVAL:align', k=(3, 3), bad='align-out'), G('EINVAL:align', bad='align-in'),
    G('EINVAL:align', minor=4, bad='align-out'), G('EINVAL:align', 'ex', ex='nof32+split+cs', minor=32, bad='align-cs'),
    G('EINVAL:align', 'ex', ex='nof32+split+cs', bad='align-cs'),
]
REQUIRED_GATES = {'null', 'size', 'empty', 'tail-null', 'tail-off-k4', 'tail-noise', 'tail-bias', 'tail-fields', 'ex-minor', 'split-args',
                  'out-null', 'adj', 'minor', 'major', 'lds', 'align'}
BYID = {c.id: c for c in CASES + GATES}
PLAIN = [c for c in CASES if c.entry == 'f32' and c.major < 1000]
DEVICE = [(c, 'exact') for c in CASES] + [(c, 'order') for c in PLAIN]


# ----------------------------------------------------------------------------------------------------------- inputs
def asym_taps(key, kh, kw):
    """The distinct integers +-1 ... +-kh*kw in a seeded order with seeded signs."""
    gen = torch.Generator(device='cpu')
    gen.manual_seed(1 + sum(key.encode()) * 7919 % 100003)
    v = (torch.randperm(kh * kw, generator=gen) + 1).float() * (torch.randint(0, 2, (kh * kw,), generator=gen).float() * 2 - 1)
    if kh * kw > 1:
        v[0], v[1] = v[0].abs(), -v[1].abs()
    return v.view(kh, kw)


def assert_asymmetric(t, what):
    kh, kw = t.shape
    assert t.unique().numel() == kh * kw and bool((t != 0).all()), what
    assert kh * kw == 1 or float(t.min()) < 0 < float(t.max()), what
    assert kw == 1 or not torch.equal(t, t.flip(1)), f'{what}: taps equal their x-flip'
    assert kh == 1 or not torch.equal(t, t.flip(0)), f'{what}: taps equal their y-flip'
    assert kh != kw or kh == 1 or not torch.equal(t, t.t()), f'{what}: taps equal their transpose'
    assert kh * kw == 1 or not torch.equal(t, t.flip(0, 1)), f'{what}: taps equal their point reflection'


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


@functools.lru_cache(maxsize=3)
def _inputs(cid, mode):
    """Operands (fp32, CPU, [major, H, W, minor]) and the fp64 expectation of everything the launch writes."""
    c = BYID[cid]
    x, kh, kw = ex_flags(c), *c.k
    sid = 'ufdf/' + c.tag
    oh, ow = out_hw(c.H, c.W, kh, kw, c.up, c.down, c.pad)
    b = case(oh=oh, ow=ow, bias=None, noise=None, nw=None, pre=None, cs=None, ref=None, b0=None, b1=None, coef=1.0, rows=None, img=None)
    oshape = (c.major, oh, ow, c.minor)
    if mode == 'order':
        b.x, b.taps = synth_tensor(sid + '/x', (c.major, c.H, c.W, c.minor)), synth_tensor(sid + '/k', (kh, kw))
        return b
    b.x, b.taps = ints(sid + '/x', (c.major, c.H, c.W, c.minor), c.amp), asym_taps(sid, kh, kw)
    assert_asymmetric(b.taps, c.id)
    v = nhwc(R.upfirdn2d_f64(nchw(b.x), b.taps, c.up, c.down, c.pad))
    assert tuple(v.shape) == oshape, (c.id, tuple(v.shape), oshape)
    budget, unit = c.amp * float(b.taps.abs().sum()), 1.0          # sum |terms| in units of the smallest power of two in play
    if c.tail:
        if 'b' in c.tail:
            b.bias = ints(sid + '/b', (c.minor,), 5)
            budget += 5
        if 'n' in c.tail.lower():
            b.noise, b.nw = ints(sid + '/n', (c.major if 'N' in c.tail else 1, oh, ow), 3), torch.tensor([NW])
            budget += 3 * NW
        v = nhwc(R.tail_f64(nchw(v), b.bias, b.noise, NW, 'a' in c.tail, SLOPE, GAIN))
        if 'a' in c.tail:
            budget, unit = budget * GAIN, unit * SLOPE * min(GAIN, 1.0)
    if 'adj' in x:
        gen = torch.Generator(device='cpu')
        gen.manual_seed(len(sid))
        b.ref = torch.tensor([3.0, -2.0, 0.0, -0.0])[torch.randint(0, 4, oshape, generator=gen)]
        v = nhwc(R.adjoint_f64(nchw(v), nchw(b.ref), ADJ_SLOPE, ADJ_GAIN))
        budget, unit = budget * ADJ_GAIN, unit * ADJ_SLOPE
        if 'part' in x:
            t = 16 if c.t16 else 8
            b.rows = R.tile_sums_f64(nchw(v), t, t).reshape(-1, c.minor)
            budget *= t * t
    assert budget / unit < 2 ** 24, f'{c.id}: sum |terms| <= {budget / unit} units: not exact in fp32'
    if 'acc' in x:
        b.pre = ints(sid + '/pre', oshape, 9)
        v = v + b.pre.double()
        assert (budget / (256 if b.rows is not None and c.t16 else 64 if b.rows is not None else 1) + 9) / unit < 2 ** 24
    b.out = v
    assert torch.equal(v.float().double(), v) and not bool((v == SENT).any()) and float(v.min()) < 0 < float(v.max()), c.id
    if 'split' in x:
        img = v
        if 'cs' in x:
            b.cs = scales(sid + '/cs', (c.major, c.minor), 'exact')
            img = v * b.cs.double()[:, None, None, :]
        top = float(img.abs().max())
        b.coef = 3.0 if 'c3' in x else 0.5
        need = math.ceil(top / b.coef) + 1 if 'low' not in x else max(1, math.floor(top / 16 / b.coef))
        b.b0, b.b1 = (need - need // 3, need // 3) if 'b1' in x else (need, None)
        b.bound = float(np.float32(b.coef) * np.float32(b.b0 + (b.b1 or 0)))
        assert b.b0 + (b.b1 or 0) < 2 ** 22 and ('low' in x or b.bound >= top)
        b.e = 13 - math.floor(math.log2(b.bound))
        b.img = img
        if 'low' not in x:         # the image is exact: hi + lo hold every value (22 bits below 2**14 after the scale)
            w = img.float() * 2.0 ** b.e
            hi = w.half()
            lo = (w - hi.float()).half()
            assert torch.equal((hi.double() + lo.double()) * 2.0 ** -b.e, img) and float(w.abs().max()) < 2 ** 14, f'{c.id}: hi + lo cannot hold the image'
        else:
            assert top * 2.0 ** b.e >= 65504
    return b


def inputs(c, mode='exact'):
    return _inputs(c.id, mode)


# ---------------------------------------------------------------------------------------------------- host-only tests
def _feat(c, P):
    """The coverage items one case reaches, named from the replay (REQUIRED lists what the table must reach together)."""
    x, f = ex_flags(c), set()
    oh, ow = P.oh, P.ow
    if P.kernel in (K4_T8, K4_T16, K4_D2):
        inst = f'k4<d{2 if P.kernel == K4_D2 else 1},{P.toh}x{P.tow},cb{P.cb4}>'
        f.add(inst + ('/tail' if c.tail else '/notail') + ('/xo' if c.entry == 'ex' else '/noxo'))
        tx = cdiv(ow, P.tow)
        f |= {f'k4:C{c.minor}', f'k4:N{c.major}', 'k4:ragged-both' if oh % P.toh and ow % P.tow else '',
              'k4:exact-multiple' if oh % P.toh == 0 and ow % P.tow == 0 else '',
              inst + ':re-dealt, tiles_x != 8' if P.gx % 8 == 0 and tx != 8 else '', inst + ':not re-dealt' if P.gx % 8 else '',
              'k4:input < tile' if c.H < P.tih and c.W < P.tiw else '', 'k4:in_h=1' if c.H == 1 else '',
              'k4:four pads' if len(set(c.pad)) == 4 else '', 'k4:negative pads' if min(c.pad) < 0 else '', 'k4:pad > 3' if max(c.pad) > 3 else ''}
        if c.tail:
            f |= {'tail:' + {'b': 'bias only', 'n': 'noise only', 'bn': 'both'}[c.tail.lower().replace('a', '')],
                  'tail:act' if 'a' in c.tail else 'tail:no act', 'tail:nb=N' if 'N' in c.tail else 'tail:nb=1' if 'n' in c.tail else ''}
        if 'adj' in x:
            f |= {'adj:t16' if c.t16 else '', 'adj:ragged' if oh % P.toh or ow % P.tow else ''}
            f.add('adj:t8, re-dealt' if not c.t16 and P.gx % 8 == 0 else 'adj:t8, not re-dealt' if not c.t16 else '')
            f.add('adj:partials' if 'part' in x else '')
    elif P.kernel == NHWC:
        kh, kw = c.k
        f |= {f'nhwc:cb{P.cb4}', 'nhwc:xo' if c.entry == 'ex' else 'nhwc:noxo', 'nhwc:up_x != up_y' if c.up[0] != c.up[1] else '',
              'nhwc:1x4' if c.k == (1, 4) else '', 'nhwc:4x1' if c.k == (4, 1) else '', 'nhwc:kh != kw' if kh != kw else '',
              'nhwc:t8x8' if (P.toh, P.tow) == (8, 8) else '', 'nhwc:shrunk, non-square' if P.toh != P.tow else '',
              'nhwc:1x1 under 60 KB' if (P.toh, P.tow) == (1, 1) and P.lds <= 60 * 1024 else '',
              'nhwc:1x1 between 60 and 64 KB' if (P.toh, P.tow) == (1, 1) and P.lds > 60 * 1024 else ''}
        if c.minor % 64 == 0:      # exactly one condition of the 4x4 gate fails
            fails = [kh != 4 or kw != 4, c.up != (1, 1), c.down[0] == c.down[1] and c.down[0] > 2, c.down[0] != c.down[1]]
            if sum(fails) == 1:
                f.add('gate:' + ('taps', 'up', 'down 3', 'down_x != down_y')[fails.index(True)])
        elif c.minor == 32 and c.k == (4, 4) and c.up == (1, 1) and c.down == (1, 1):
            f.add('gate:minor 32')
    else:
        f |= {'planar:16x64' if (P.toh, P.tow) == (16, 64) else 'planar:shrunk', 'planar:slab loop' if P.launches > 1 else '',
              f'planar:off{c.off}' if c.off else '', 'planar:several tiles' if P.gx > 1 else ''}
        for tag, up, down, p0, p1, n, ch, h, w, ks in UPFIRDN_CASES:
            if (c.H, c.W, c.k, c.up, c.down, c.pad) == (h, w, (ks, ks), (up, up), (down, down), (p0, p1, p0, p1)):
                f.add('planar:golden geometry')
    if c.entry == 'ex':
        f |= {'ex:accumulate' if 'acc' in x else '', 'ex:no_f32, out stays' if 'nof32' in x and 'null' not in x else '',
              'ex:no_f32, out NULL, split' if {'nof32', 'null', 'split'} <= x else '', 'ex:amax' if 'amax' in x else '',
              'ex:low bound' if 'low' in x else ''}
        if 'split' in x:
            f |= {'split:bound1' if 'b1' in x else 'split:no bound1', 'split:coef 3' if 'c3' in x else 'split:coef 0.5',
                  'split:chan_scale' if 'cs' in x else 'split:no chan_scale', f'split:minor {c.minor}'}
    f.discard('')
    return f


_K4 = ('k4<d1,8x8,cb16>', 'k4<d1,16x16,cb8>', 'k4<d2,4x8,cb16>')
REQUIRED = (
    {i + t + x for i in _K4 for t in ('/tail', '/notail') for x in ('/xo', '/noxo')}
    | {i + s for i in _K4 for s in (':re-dealt, tiles_x != 8', ':not re-dealt')}
    | {'k4:C64', 'k4:C128', 'k4:N1', 'k4:N3', 'k4:ragged-both', 'k4:exact-multiple', 'k4:input < tile', 'k4:in_h=1', 'k4:four pads',
       'k4:negative pads', 'k4:pad > 3', 'tail:bias only', 'tail:noise only', 'tail:both', 'tail:act', 'tail:no act', 'tail:nb=N', 'tail:nb=1',
       'adj:t16', 'adj:ragged', 'adj:t8, re-dealt', 'adj:t8, not re-dealt', 'adj:partials',
       'ex:accumulate', 'ex:no_f32, out stays', 'ex:no_f32, out NULL, split', 'ex:amax', 'ex:low bound', 'split:bound1', 'split:no bound1',
       'split:coef 3', 'split:coef 0.5', 'split:chan_scale', 'split:no chan_scale', 'split:minor 32', 'split:minor 64', 'split:minor 128',
       'nhwc:cb1', 'nhwc:cb2', 'nhwc:cb8', 'nhwc:cb16', 'nhwc:xo', 'nhwc:noxo', 'nhwc:up_x != up_y', 'nhwc:1x4', 'nhwc:4x1', 'nhwc:kh != kw',
       'nhwc:t8x8', 'nhwc:shrunk, non-square', 'nhwc:1x1 under 60 KB', 'nhwc:1x1 between 60 and 64 KB',
       'gate:taps', 'gate:up', 'gate:down 3', 'gate:down_x != down_y', 'gate:minor 32',
       'planar:16x64', 'planar:shrunk', 'planar:slab loop', 'planar:off1', 'planar:off2', 'planar:off3', 'planar:several tiles',
       'planar:golden geometry'})


def touched(o, down, k, up, pad0):
    """Input samples (not clipped to the input) that output o of an axis reads, from the definition: it reads the canvas positions
    o * down ... o * down + k - 1, and canvas position q holds sample i iff q - pad0 == i * up."""
    return [(q - pad0) // up for q in range(o * down, o * down + k) if (q - pad0) % up == 0]


def window_covers(P, up, down, pad, k):
    """The staged window [lo, lo + tih) x [lo, lo + tiw) of the first, a middle and the last tile holds what their outputs read."""
    for n, t, ti, u, d, p0, kk in ((P.oh, P.toh, P.tih, up[1], down[1], pad[2], k[0]), (P.ow, P.tow, P.tiw, up[0], down[0], pad[0], k[1])):
        nt = cdiv(n, t)
        for tile in {0, nt // 2, nt - 1}:
            o0 = tile * t
            lo = -(-(o0 * d - p0) // u)       # the first sample at or after the tile's first canvas position, o0 * down
            for o in range(o0, min(o0 + t, n)):
                if any(not lo <= i < lo + ti for i in touched(o, d, kk, u, p0)):
                    return False
    return True


def sweep_geometries(n=4000):
    rnd = random.Random(19)
    for _ in range(n):
        minor = rnd.choice([1, 1, 1, 3, 4, 8, 12, 32, 64, 64, 64, 72, 128, 192])
        k4 = rnd.random() < 0.4
        kh, kw = (4, 4) if k4 else (rnd.randint(1, 16), rnd.randint(1, 16))
        up = (1, 1) if k4 and rnd.random() < 0.8 else (rnd.randint(1, 3), rnd.randint(1, 3))
        d = rnd.choice([1, 1, 2, 2, 3, 8])
        down = (d, d) if rnd.random() < 0.7 else (rnd.randint(1, 4), rnd.randint(1, 4))
        pad = tuple(rnd.randint(-3, 9) for _ in range(4))
        major = rnd.choice([1, 2, 3, 5, 7, 16, 300, 65535, 65536, 140000])
        yield (major, rnd.randint(1, 70), rnd.randint(1, 70), minor, kh, kw, up, down, pad, rnd.random() < 0.12, rnd.random() < 0.25, rnd.random() < 0.9)


def held_to_library(args, t16, what):
    from rick_amd._lib import lib
    major, H, W, minor, kh, kw, up, down, pad, has_tail, has_ex, aligned16 = args
    why, P = plan_replay(major, H, W, minor, kh, kw, up, down, pad, has_tail, has_ex, aligned16, t16)
    rc, got = lib_plan(major, H, W, minor, kh, kw, up, down, pad, has_tail, has_ex, aligned16)
    if why:
        assert rc == EINVAL and got == [-1] * 12, f'{what}: the replay refuses ({why}), rick_upfirdn2d_plan returns {rc} {got}'
        return None
    assert rc == 0 and got == fields(P), f'{what}: rick_upfirdn2d_plan says {rc} {got}, the replay {fields(P)}'
    assert P.lds <= 64 * 1024 and P.gy <= 65535 and P.gz <= 65535 and (P.launches == 1 or P.kernel == PLANAR), what
    assert window_covers(P, up, down, pad, (kh, kw)), f'{what}: the staged window misses an input row or column'
    if P.kernel in (K4_T8, K4_T16):
        assert lib.rick_upfirdn2d_adjoint_rows(major, P.oh, P.ow) == major * P.gx, f'{what}: rick_upfirdn2d_adjoint_rows'
    return P


def plan_args(c):
    why, _ = replay(c)
    x = ex_flags(c)
    aligned16 = c.bad not in ('align-in', 'align-out', 'align-cs') and c.off % 4 == 0
    return (c.major, c.H, c.W, c.minor, *c.k, c.up, c.down, c.pad, bool(c.tail), c.entry == 'ex' and c.bad != 'ex-null', aligned16)


PLAN_GATES = {'size', 'empty', 'tail-off-k4', 'minor', 'align', 'lds', 'major', 'ex-planar', 'grid'}


def test_case_ids_replay_and_library_agree():
    """No device.  Every case's literal `want` is what the replayed entry gates and planner give; the replay is the library's own
    plan on every case and on the sweep, under both values of the tile-16 switch; rick_upfirdn2d_adjoint_rows agrees with both;
    the staged window covers what the tile's outputs read (from the definition); the table reaches the whole coverage list and
    every gate; the size caps hold."""
    from rick_amd._lib import lib
    assert len(BYID) == len(CASES + GATES)
    reached, gates = set(), set()
    for c in CASES + GATES:
        with tile16(c.t16):
            P, want = want_of(c)
            assert want == c.want, f'{c.id}: the replay reaches {want}'
            why, _ = replay(c)
            if why is None or why in PLAN_GATES:
                assert held_to_library(plan_args(c), c.t16, c.id) is None or why is None, c.id
        if c in CASES:
            assert P is not None and not c.bad, c.id
            reached |= _feat(c, P)
            if c.major < 1000:
                assert max(c.H, c.W) <= 70 and c.major <= 6 and c.minor <= 128, c.id
            assert c.major * max(c.H * c.W, P.oh * P.ow) * c.minor <= 600_000, c.id
        else:
            assert P is None, c.id
            gates.add(why)
    assert not REQUIRED - reached, f'not reached: {sorted(REQUIRED - reached)}'
    have = {(c.H, c.W, c.k, c.up, c.down, c.pad) for c in CASES if c.minor == 1}
    for tag, up, down, p0, p1, n, ch, h, w, ks in UPFIRDN_CASES:
        assert (h, w, (ks, ks), (up, up), (down, down), (p0, p1, p0, p1)) in have, f'no planar case on the golden geometry {tag}'
    assert not REQUIRED_GATES - gates, f'gates not reached: {sorted(REQUIRED_GATES - gates)}'
    # what the issue states by reading the code: 14 x 15 taps on 64 channels -> the 1x1 tile between 60 and 64 KB; 16 x 16 taps, up 1 -> refused
    why, P = plan_replay(1, 3, 3, 64, 14, 15, (1, 1), (1, 1), (7, 7, 7, 7), False, False, True, 0)
    assert (P.toh, P.tow) == (1, 1) and 60 * 1024 < P.lds <= 64 * 1024
    assert plan_replay(1, 3, 3, 64, 16, 16, (1, 1), (1, 1), (8, 8, 8, 8), False, False, True, 0)[0] == 'lds'
    kinds = {}
    for t16 in (0, 1):
        with tile16(t16):
            for g in sweep_geometries():
                P = held_to_library(g, t16, f'{g} tile16={t16}')
                k = 'refused' if P is None else f'{P.kernel}:{P.toh}x{P.tow}' + ('/slabs' if P.launches > 1 else '')
                kinds[k] = kinds.get(k, 0) + 1
        assert lib.rick_conv_tuning(TUNE_UFD_TILE16, 0) == 0, 'the switch was not put back'
    print(f'forms of the sweep: {sorted(kinds.items())}')
    assert {'0:8x8', '1:16x16', '2:4x8', '3:8x8', '3:1x1', '4:16x64', '4:16x64/slabs', 'refused'} <= set(kinds)
    assert lib.rick_upfirdn2d_plan(1, 8, 8, 64, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, None) == EINVAL


def test_reference_meets_the_goldens_and_the_c_oracle(golden):
    """No device.  tests/ufd_f64.py against the committed reference-derived results (y of every UPFIRDN_CASES tag, at the tolerance
    of tests/test_oracle_vs_golden.py) and against the scalar C oracle on anisotropic geometries with integer data: equal."""
    from oracle import c_ref
    g = golden('ops')
    for tag, up, down, p0, p1, n, ch, h, w, ks in UPFIRDN_CASES:
        x = synth_tensor(f'upfirdn/{tag}/x', (n, ch, h, w)).double()
        y = R.upfirdn2d_f64(x, upfirdn_kernel(ks, up).double(), (up, up), (down, down), (p0, p1, p0, p1)).numpy()
        want = g[f'{tag}/y']
        assert y.shape == want.shape and np.abs(y - want).max() <= 1e-13 * np.abs(want).max(), tag
    rnd = random.Random(7)
    for i in range(60):
        kh, kw = rnd.randint(1, 6), rnd.randint(1, 6)
        up, down = (rnd.randint(1, 3), rnd.randint(1, 3)), (rnd.randint(1, 3), rnd.randint(1, 3))
        pad = tuple(rnd.randint(-2, 5) for _ in range(4))
        h, w = rnd.randint(3, 11), rnd.randint(3, 11)
        if (h * up[1] + pad[2] + pad[3] - kh) < 0 or (w * up[0] + pad[0] + pad[1] - kw) < 0:
            continue
        x, t = ints(f'ufdf/oracle/{i}', (2, 3, h, w), 9), asym_taps(f'o{i}', kh, kw)
        y = R.upfirdn2d_f64(x, t, up, down, pad)
        yc = c_ref.upfirdn2d_c(x.numpy(), t.numpy(), up, down, pad)
        assert tuple(y.shape) == yc.shape and np.array_equal(y.numpy(), yc.astype(np.float64)), (kh, kw, up, down, pad, h, w)
    # the helpers, on values one can check by hand
    v = torch.tensor([[[[-4.0, 2.0], [0.0, 6.0]]]])
    assert R.tail_f64(v, torch.tensor([1.0]), torch.tensor([[[1.0, -1.0], [0.0, 2.0]]]), 3.0, True, 0.25, 2.0).flatten().tolist() == [0.0, 0.0, 2.0, 26.0]
    assert R.adjoint_f64(v, torch.tensor([[[[1.0, -1.0], [0.0, -0.0]]]]), 0.5, 2.0).flatten().tolist() == [-8.0, 2.0, 0.0, 6.0]
    assert R.tile_sums_f64(torch.arange(12.0).view(1, 1, 3, 4), 2, 3).flatten().tolist() == [0 + 1 + 2 + 4 + 5 + 6, 3 + 7, 8 + 9 + 10, 11]


def test_exact_inputs_fit():
    """No device.  Every exact-mode builder passes its own assertions: asymmetric taps, sum |terms| < 2**24 units, results that are
    fp32 numbers of both signs and never the sentinel, split images that hi + lo hold exactly."""
    for c in CASES:
        if c.major < 1000:
            inputs(c)
    assert len(DEVICE) + len(GATES) <= 200


# ----------------------------------------------------------------------------------------------------- device helpers
def word_of(value):
    w = torch.zeros(AMAX_FLOATS)
    w[5 * AMAX_STRIDE] = float(value)
    return fenced(w)


def launch(c, b, mode='exact'):
    """One launch into fresh guarded buffers -> rc and the buffers (`c.bad` misaligns an operand or takes it away)."""
    from rick_amd._lib import ConvEpilogue, SplitOut, lib
    x, bad = ex_flags(c), c.bad
    numel = c.major * b.oh * b.ow * c.minor
    o = case(keep=[])
    o.x = fenced(b.x, c.off + (1 if bad == 'align-in' else 0))
    o.k = fenced(b.taps)
    o.out = Guarded(numel + 4)
    o.ooff = c.off + (1 if bad == 'align-out' else 0)
    if 'acc' in x and b.pre is not None:
        o.out.v[o.ooff:o.ooff + numel].copy_(b.pre.reshape(-1))
    o.prefill = o.out.buf.clone()
    outp = None if 'null' in x or bad == 'null-out' else o.out.v[o.ooff:].data_ptr()
    tail = None
    if c.tail:
        tail = ConvEpilogue()
        o.bias, o.noise, o.nw = fenced(b.bias, 1 if bad == 'bias-align' else 0), fenced(b.noise), fenced(b.nw)
        tail.bias, tail.noise, tail.noise_w = p(o.bias), p(o.noise), None if bad == 'noise-now' else p(o.nw)
        tail.noise_nb = (c.major + 1 if bad == 'noise-nb' else b.noise.shape[0]) if b.noise is not None else 1
        tail.act, tail.slope, tail.gain = int('a' in c.tail), SLOPE, GAIN
        if bad in ('tail-amax', 'tail-split'):
            o.tword = Guarded(AMAX_FLOATS)
            setattr(tail, 'amax' if bad == 'tail-amax' else 'split_out', p(o.tword))
    ex = None
    o.word = o.img = o.hdr = o.part = None
    if c.entry == 'ex' and bad != 'ex-null':
        ex = SplitOut()
        ex.bound_coef = 1.0
        ex.accumulate, ex.no_f32 = int('acc' in x), int('nof32' in x)
        if 'amax' in x:
            o.word = Guarded(AMAX_FLOATS, torch.zeros(AMAX_FLOATS))
            ex.amax = p(o.word)
        if 'split' in x:
            o.img, o.hdr = Guarded(numel + 4), Guarded(4)
            o.w0, o.w1 = word_of(b.b0 if b.b0 is not None else 1.0), (word_of(b.b1) if b.b1 is not None else None)
            ex.split_out = o.img.v[(1 if bad == 'split-align' else 0):].data_ptr()
            ex.split_hdr = None if bad == 'split-nohdr' else p(o.hdr)
            ex.bound0, ex.bound1 = None if bad == 'split-nobound' else p(o.w0), p(o.w1)
            ex.bound_coef = 0.0 if bad == 'split-coef' else b.coef
            if 'cs' in x:
                o.cs = fenced(b.cs if b.cs is not None else torch.ones(c.major, c.minor), 1 if bad == 'align-cs' else 0)
                ex.chan_scale = p(o.cs)
        if 'adj' in x:
            o.ref = fenced(b.ref if b.ref is not None else torch.ones(max(numel, 4)), 1 if bad == 'adj-align' else 0)
            ex.adj_ref, ex.adj_slope, ex.adj_gain = p(o.ref), ADJ_SLOPE, ADJ_GAIN
            if 'part' in x:
                o.nrows = lib.rick_upfirdn2d_adjoint_rows(c.major, b.oh, b.ow)
                o.part = Guarded(o.nrows * c.minor + 4)
                ex.adj_partials = o.part.v[(1 if bad == 'part-align' else 0):].data_ptr()
    geo = (c.major, c.H, c.W, c.minor, *c.k, c.up[0], c.up[1], c.down[0], c.down[1], *c.pad)
    args = (None if bad == 'null-in' else p(o.x), None if bad == 'null-k' else p(o.k), outp) + geo
    if c.entry == 'f32':
        o.rc = lib.rick_upfirdn2d_f32(*args, stream())
    elif c.entry == 'act':
        o.rc = lib.rick_upfirdn2d_act_f32(*args, ctypes.byref(tail) if tail else None, stream())
    else:
        o.rc = lib.rick_upfirdn2d_ex_f32(*args, ctypes.byref(tail) if tail else None, ctypes.byref(ex) if ex else None, stream())
    torch.cuda.synchronize()
    for what, gd in (('out', o.out), ('amax word', o.word), ('split image', o.img), ('header', o.hdr), ('adj_partials', o.part)):
        if gd is not None:
            gd.assert_bands(f'{c.id} {what}')
    return o


def same(dev, exp, what):
    """torch.equal with a report of where and by how much."""
    wrong = dev != exp
    if bool(wrong.any()):
        at = wrong.nonzero()
        d = (dev.double() - exp.double())[wrong].abs()
        raise AssertionError(f'{what}: {int(wrong.sum())} of {wrong.numel()} elements differ, by {float(d.min())} .. {float(d.max())}; first at '
                             f'{tuple(at[0].tolist())}: {float(dev[wrong][0])} != {float(exp[wrong][0])}; images {sorted(set(at[:, 0].tolist()))[:6]}, '
                             f'rows {sorted(set(at[:, 1].tolist()))[:8]}, cols {sorted(set(at[:, 2].tolist()))[:8]}' if at.shape[1] >= 3 else
                             f'{what}: {int(wrong.sum())} of {wrong.numel()} elements differ, first at {tuple(at[0].tolist())}: '
                             f'{float(dev[wrong][0])} != {float(exp[wrong][0])}')


def check(c, b, o, mode):
    x = ex_flags(c)
    numel = c.major * b.oh * b.ow * c.minor
    shape = (c.major, b.oh, b.ow, c.minor)
    assert o.rc == 0, f'{c.id}: rc = {o.rc}'
    outside = torch.ones_like(o.out.buf, dtype=torch.bool)
    lo = o.out.lo + o.ooff
    outside[lo:lo + numel] = False
    assert torch.equal(o.out.buf[outside], o.prefill[outside]), f'{c.id}: wrote outside the output'
    dev = o.out.buf[lo:lo + numel].cpu().view(shape)
    if 'nof32' in x:
        assert o.out.untouched(), f'{c.id}: no_f32, and the fp32 output was written'
    elif mode == 'order':
        from oracle import c_ref
        yc = torch.from_numpy(c_ref.upfirdn2d_c(nchw(b.x).contiguous().numpy(), b.taps.numpy(), c.up, c.down, c.pad))
        same(dev.view(torch.int32), nhwc(yc).view(torch.int32), f'{c.id}: bits against the C oracle')
    else:
        assert not bool(torch.isnan(dev).any()), f'{c.id}: NaN in the result'
        same(dev, b.out.float(), c.id)
    if o.word is not None:
        amax_word_check(o.word.v.cpu(), float(b.out.abs().max()), c.id)
    if o.img is not None:
        hdr = o.hdr.v.cpu()
        assert hdr.tolist() == [2.0 ** b.e, 2.0 ** -b.e, b.bound, 0.0], f'{c.id}: header {hdr.tolist()}, expected 2^{b.e}, 2^-{b.e}, {b.bound}, 0'
        assert bool((o.img.v[numel:] == SENT).all())
        if 'low' not in x:
            got = decode_image(o.img.v[:numel].cpu(), hdr).view(shape)
            assert not bool(torch.isnan(got).any()), f'{c.id}: NaN in the image'
            same(got, b.img.float(), f'{c.id}: split image')
    if o.part is not None:
        assert o.nrows == b.rows.shape[0], f'{c.id}: rick_upfirdn2d_adjoint_rows = {o.nrows}, the tiles are {b.rows.shape[0]}'
        same(o.part.v[:o.nrows * c.minor].cpu().view(o.nrows, c.minor), b.rows.float(), f'{c.id}: adj_partials rows')
        assert bool((o.part.v[o.nrows * c.minor:] == SENT).all())


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@pytest.mark.parametrize('c,mode', DEVICE, ids=[f'{c.id}-{m}' for c, m in DEVICE])
def test_ufd_forms(c, mode):
    from rick_amd._lib import lib
    low = 'low' in ex_flags(c)
    with tile16(c.t16):
        P, want = want_of(c)
        assert want == c.want and P is not None
        b = inputs(c, mode)
        sat0 = sat_count()
        try:
            o = launch(c, b, mode)
            check(c, b, o, mode)
            if low:
                assert sat_count() > sat0, f'{c.id}: a bound 16x too small, and the saturation count did not move'
            else:
                assert sat_count() == sat0, f'{c.id}: the saturation count moved'
        finally:
            if low:
                cnt = ctypes.c_uint(0)
                lib.rick_saturation_count(ctypes.byref(cnt), 1)
    assert not low or sat_count() == 0


@gpu
@pytest.mark.parametrize('c', GATES, ids=[c.id for c in GATES])
def test_ufd_refuses_on_the_host(c):
    """RICK_EINVAL before anything is launched: every buffer the call could write keeps its sentinels."""
    P, want = want_of(c)
    assert want == c.want and P is None
    kh, kw = max(c.k[0], 1), max(c.k[1], 1)
    oh, ow = out_hw(max(c.H, 1), max(c.W, 1), kh, kw, (max(c.up[0], 1), max(c.up[1], 1)), (max(c.down[0], 1), max(c.down[1], 1)), c.pad)
    oh, ow = max(oh, 1), max(ow, 1)
    major, minor = max(c.major, 1), max(c.minor, 1)
    b = case(oh=oh, ow=ow, x=torch.ones(major, max(c.H, 1), max(c.W, 1), minor), taps=torch.ones(kh, kw), bias=torch.ones(minor),
             noise=torch.ones(major if 'N' in c.tail else 1, oh, ow) if 'n' in c.tail.lower() else None, nw=torch.ones(1), pre=None, cs=None,
             ref=None, b0=None, b1=None, coef=1.0)
    o = launch(c, b)
    assert o.rc == EINVAL, f'{c.id}: rc = {o.rc}'
    for gd in (o.out, o.img, o.hdr, o.part, getattr(o, 'tword', None)):
        assert gd is None or gd.untouched(), f'{c.id}: refused, and something was written'
    assert o.word is None or bool((o.word.v == 0).all())


ANY = [('f64', 1, 3, 9, 11, (4, 3), (2, 1), (1, 2), (2, 1, 0, 3)), ('f16-int', 2, 3, 9, 11, (3, 4), (1, 2), (2, 1), (1, 2, 2, 0)),
       ('f16-round', 2, 2, 12, 10, (4, 4), (1, 1), (1, 1), (2, 1, 1, 2)), ('grid-stride', 2, 1, 4100, 4100, (1, 2), (1, 1), (1, 1), (0, 0, 0, 0))]


@gpu
@pytest.mark.parametrize('name,dtype,major,H,W,k,up,down,pad', ANY, ids=[a[0] for a in ANY])
def test_ufd_any_forms(name, dtype, major, H, W, k, up, down, pad):
    """rick_upfirdn2d_any (planar): fp64 meets the reference exactly; fp16 with integer results of at most 2048 exactly, with
    results that need the one rounding the fp64 result rounded once to half; more than 65535 x 256 outputs enter the grid-stride loop."""
    from rick_amd._lib import lib
    td = torch.float64 if dtype == 1 else torch.float16
    taps = asym_taps('any/' + name, *k) if name != 'grid-stride' else torch.tensor([[3.0, -5.0]])
    if name == 'f16-round':
        x, taps = ints('ufdf/any/x/' + name, (major, 1, H, W), 40) + 0.5, taps * 0.25 + 1.0
    else:
        x = ints('ufdf/any/x/' + name, (major, 1, H, W), 8 if dtype == 2 else 1000)
    assert torch.equal(x.to(td).double(), x.double()) and torch.equal(taps.to(td).double(), taps.double())
    ref = R.upfirdn2d_f64(x, taps, up, down, pad)
    top = float(ref.abs().max())
    if name == 'f16-round':
        assert bool((ref.half().double() != ref).any()) and top < 60000 and 40.5 * float(taps.abs().sum()) < 2 ** 24 * 2.0 ** -3
    elif dtype == 2:
        assert top <= 2048 and float(ref.min()) < 0 < float(ref.max())
    n = ref.numel()
    assert (n > 65535 * 256) == (name == 'grid-stride')
    bx = torch.full((x.numel() + 128,), float('nan'), dtype=td, device=DEV)
    bx[64:64 + x.numel()] = x.reshape(-1).to(td)
    bk = torch.full((taps.numel() + 128,), float('nan'), dtype=td, device=DEV)
    bk[64:64 + taps.numel()] = taps.reshape(-1).to(td)
    out = torch.full((n + 128,), SENT, dtype=td, device=DEV)
    sent = out[0].clone()
    sat0 = sat_count()
    rc = lib.rick_upfirdn2d_any(bx[64:].data_ptr(), bk[64:].data_ptr(), out[64:].data_ptr(), dtype, major, H, W, *k, *up, *down, *pad, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((out[:64] == sent).all()) and bool((out[64 + n:] == sent).all()), f'{name}: wrote outside the output'
    exp = ref.to(td).reshape(-1).to(DEV)            # fp64 -> half: one rounding to nearest even
    got = out[64:64 + n]
    assert not bool(torch.isnan(got).any())
    bad = (got != exp).nonzero()
    assert bad.numel() == 0, f'{name}: {bad.shape[0]} of {n} differ, first at {int(bad[0])}: {float(got[bad[0]])} != {float(exp[bad[0]])}'
    assert sat_count() == sat0
    assert lib.rick_upfirdn2d_any(bx[64:].data_ptr(), bk[64:].data_ptr(), out[64:].data_ptr(), 0, major, H, W, *k, *up, *down, *pad, stream()) == EINVAL
    assert lib.rick_upfirdn2d_any(bx[64:].data_ptr(), bk[64:].data_ptr(), out[64:].data_ptr(), 3, major, H, W, *k, *up, *down, *pad, stream()) == EINVAL


OPS = [('blur', 64, 1, (2, 1)), ('decimate', 64, 2, (2, 2)), ('planar', 3, 1, (2, 1)), ('planar-down2', 3, 2, (1, 1)), ('fused', 64, 1, (2, 1)),
       ('fused-128', 128, 1, (1, 2))]


@gpu
@pytest.mark.parametrize('name,C_,down,pad', OPS, ids=[o[0] for o in OPS])
def test_ufd_python_ops_exact(name, C_, down, pad):
    """rick_amd.op.upfirdn2d / upfirdn2d_noise_bias_act with asymmetric integer 4x4 taps: the forward, gx and ggy equal fp64 autograd
    of the reference exactly (the adjoint flips the taps and exchanges up and down: down 2 runs the up-2 generic kernel)."""
    from rick_amd import op
    N, H, W = 2, 13, 10
    taps = asym_taps('op/' + name, 4, 4)
    assert_asymmetric(taps, name)
    x = ints('ufdf/op/x/' + name, (N, C_, H, W), 4)
    fused = name.startswith('fused')
    x64 = x.double().requires_grad_(True)
    y64 = R.upfirdn2d_f64(x64, taps, (1, 1), (down, down), (pad[0], pad[1], pad[0], pad[1]))
    if fused:
        bias, noise, nw = ints('ufdf/op/b/' + name, (C_,), 5), ints('ufdf/op/n/' + name, (N, 1, y64.shape[2], y64.shape[3]), 3), torch.tensor([NW])
        y64 = R.tail_f64(y64, bias, noise.view(N, y64.shape[2], y64.shape[3]), NW, True, SLOPE, GAIN)
    gy = ints('ufdf/op/gy/' + name, tuple(y64.shape), 4)
    ggx = ints('ufdf/op/ggx/' + name, tuple(x.shape), 4)
    gy64 = gy.double().requires_grad_(True)
    (gx64,) = torch.autograd.grad(y64, x64, gy64, create_graph=True)
    (ggy64,) = torch.autograd.grad(gx64, gy64, ggx.double())
    for t in (y64, gx64, ggy64):
        assert torch.equal(t.detach().float().double(), t.detach()) and float(t.detach().abs().max()) < 2 ** 22
    xd = x.to(DEV).requires_grad_(True)
    if fused:
        y = op.upfirdn2d_noise_bias_act(xd, taps.to(DEV), pad, bias.to(DEV), noise.to(DEV), nw.to(DEV), SLOPE, GAIN)
    else:
        y = op.upfirdn2d(xd, taps.to(DEV), up=1, down=down, pad=pad)
    gyd = gy.to(DEV).requires_grad_(True)
    (gx,) = torch.autograd.grad(y, xd, gyd, create_graph=True)
    (ggy,) = torch.autograd.grad(gx, gyd, ggx.to(DEV))
    for what, dev, ref in (('forward', y, y64), ('gx', gx, gx64), ('ggy', ggy, ggy64)):
        same(dev.detach().cpu(), ref.detach().float(), f'{name}: {what}')
