"""Every dispatch form of the one-pass transposed 3x3 stride-2 convolution (rick_amd/csrc/convt2.hip), through the C ABI
(rick_conv_pack_weight with nslices = 9, rick_convt2_f32, rick_convt2_split_f32, rick_convt2_workspace_bytes, rick_convt2_plan,
rick_convt2_posmap), against the fp64 expression of include/rick_hip.h written out here:

    out[n, 2*iy+ky, 2*ix+kx, co] = alpha * oscale[n,co] * sum_ci W[ky*3+kx][co][ci] * (iscale[n,ci] * x[n,iy,ix,ci])

cropped to OH x OW (OH in {2 IH, 2 IH + 1}, likewise OW).  The op/ layer is not used.  The method and the conventions are those
of tests/test_gpu_igemm_forms.py; tests/forms_common.py holds what the two share.

The planner is replayed on the host (ct2_plan: the cost model with CT_SUB2_PCT / CT_SUB4_PCT, the 160 KB LDS gate, CT_MAX_NPP =
192, nfull / subq; ct2_position_map: the pad loop and its identity fallback; the block -> (work item, fragment columns) decode
of convt2_kernel with xcd_remap); every case states the form it reaches as a literal (`want`), which is also its id:

    ct2<s2,pk0>/NJ8+NJ2/t6x5x4/pw7-perm/s3x2/red<osc,noamax>
    instantiation <SPLIT, PKX> / launches (whole-tile blocks + sub-blocks of the last round) / tile TW x TH x NB / patch pitch
    and map kind / splits x chunks per split / second stage <oscale, amax word>

The host-only test holds the literal to the replay and the replay to the library (all 8 fields of rick_convt2_plan, the 128
entries and the pitch of rick_convt2_posmap, rick_convt2_workspace_bytes) on every case and on a sweep of 3 000 geometries
(N <= 16, IH, IW <= 48 and non-square, Ci / Co that are no multiples of 32 / 128, both OH and OW choices), and asserts the map's
invariants on the sweep from the library's output alone: the entries without bit 7 are a permutation of [0, TW*TH*NB), those
with bit 7 carry a valid position, TW + 1 <= pitch <= TW + 4, NB * (TH + 1) * pitch <= 192, LDS <= 160 KB, and the two launches
cover every (work item, fragment column) exactly once.

Each output element carries the number of terms of its own parity class, K = Ci x {4, 2, 2, 1} less what border positions lose
(counted by the same scatter as the reference, on ones).  Checks, none with a measured tolerance:

  exact11  x and W non-zero integers |v| <= amp <= 4 of mixed sign, iscale / oscale in {0.5, 1, 2}, alpha = 0.25, packer scale 1,
           and sum |terms| < 2**24 units for every output element (asserted on the CPU from an upper bound): every product,
           every partial sum in any order, the split-K `* unscale`, the reduce and the scales are exact fp32 numbers:
           torch.equal to the fp64 result cast to fp32.  Pins the position map, the tap slices and offsets of every class,
           border tiles, masks, the work-item decode of both launches.
  exact22x / exact22w  (split == 2 and the split-image entry) one operand (x / W) takes fine() values — 12 significant bits, the
           last one set — the other integers |v| <= min(amp, 2): torch.equal again.  The only mode that fails when a wave's `lo`
           fragments are dropped or misplaced (the alo reload in mma_tap, the pl buffer, the lo tile of the packed weight, the lo
           half of a split image).  Every split == 2 case runs it: the amplitudes keep Ci = 512 ... 1 024 (K up to 4 096) inside
           the budget, which is asserted, so no form is left to the bound alone (LO_BLIND is empty).
  bound    standard-normal operands, scales in [0.5, 1.5], packer scale 2**-0.5; per output element |dev - ref64| <= the a-priori
           bound of the igemm file (forms_common.bound_terms): representation 3 * 2**-22 * S (split == 1: 2 * 2**-11 * S),
           2**-27 * (Xmax sum|w| + Wmax sum|x|) below the window, accumulation (K + nsplit + R) * 2**-24 * S with the element's
           own K, and one ulp of the result.  R = 6: the packer's weight-scale product (1), the iscale product (1; the block
           exponent folded into the table is a power of two), two more additions per term (three MFMA products), and the
           output factor (2: direct store oscale * (alpha * 2^-e) and acc * that; through the reduce kernel sum * alpha and
           * oscale; acc * 2^-e is exact).  No tail here, so R is smaller than the igemm's 12.
           A bound case is launched twice: bit-identical.  The host-only test shows on the CPU that the bound sees a lost `lo`
           half on every split == 2 case with K <= 160.

Every device case: output, workspace and amax word between sentinel bands; the output is prefilled with the sentinel and no
element keeps it (every element of [N, OH, OW, Co] is written exactly once; the cropped row / column does not exist, the bands
cover it); with one split a workspace passed anyway stays untouched and NULL is accepted (the second launch); x, iscale, oscale,
the source weight, the packed weight and the split image with its header are views with NaN on both sides; the saturation
counter stays put.  Split entry with an amax word: the maximum over the 16 slots equals max |out| of the device output exactly,
with one split (cv_amax_publish in the kernel) and with several (the reduce kernel).  Exact modes: the split entry and the fp32
SPLIT = 2 entry give equal tensors on the same values.

Forms without a case.  Maps padded by 2 or 3 columns (pitch TW + 3, TW + 4): neither the sweep nor a search over 40 000 further
geometries with N <= 16 and IH, IW <= 48 reaches one (the tiles the planner picks there take pad 0, pad 1 or the identity map);
the host-only test prints the kinds the sweep reaches and fails should a pad2 / pad3 map turn up, so that it gets a case then.
The identity map and the pad1 map with all 128 slots in use: no geometry under the cap either (both appear with unused slots,
and have cases).  RICK_CT2_TILE / RICK_CT2_SUBQ and the saturation ballot exist in the ablation build only.  A host-side swap of
two map entries relabels slots consistently for the read and the store and computes the same convolution: only the host-only
test (replay against rick_convt2_posmap) sees it; a swap on the read side alone fails the exact modes.
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
from tests.forms_common import (AMAX_FLOATS, SENT, Fenced, Guarded, amax_word_check, bound_terms, cdiv, f32, fenced, fine, ints,
                                nan_fence_ok, p, rep_of, sat_count, scales, split_halves, split_image, stream)

gpu = pytest.mark.gpu
EINVAL = 22
LDS_MAX = 160 * 1024
MAX_NPP = 192                 # CT_MAX_NPP
SUB2_PCT, SUB4_PCT = 68, 64   # CT_SUB2_PCT, CT_SUB4_PCT
R_ROUND = 6                   # further roundings on a term (module docstring)
MAX_OUT_FLOATS, MAX_MACS = 3_000_000, 2e9


def case(**kw):
    return types.SimpleNamespace(**kw)


# ---------------------------------------------------------------------------------------------- host-side planner replay
@functools.lru_cache(maxsize=None)
def ct2_plan(N, IH, IW, Ci, Co, OH, OW):
    """ct2_plan and ct2_position_map -> the plan (None: RICK_EINVAL).  The three nested loops of the source run here as one
    array over (tw, th) x s in the same order; argmin keeps the first of equal costs, as `cost < best` does."""
    if min(N, IH, IW, Ci, Co) <= 0 or Ci & 3 or Co & 3:
        return None
    if not (2 * IH <= OH <= 2 * IH + 1 and 2 * IW <= OW <= 2 * IW + 1):
        return None
    if N * IH * IW * Ci >= 1 << 31 or N * OH * OW * Co >= 1 << 31:
        return None
    nchunks, ncot = cdiv(Ci, 32), cdiv(Co, 128)
    GH, GW = IH + 1, IW + 1
    pairs = np.array([(tw, th) for tw in range(1, min(GW, 128) + 1) for th in range(1, min(GH, 128 // tw) + 1)], dtype=np.int64)
    tw, th = pairs[:, 0:1], pairs[:, 1:2]
    nb = np.minimum(128 // (tw * th), N)
    npp = nb * (th + 1) * (tw + 1)
    tiles = -(-GW // tw) * -(-GH // th) * -(-N // nb) * ncot
    s = np.arange(1, min(nchunks, 16) + 1, dtype=np.int64)[None, :]
    cps = -(-nchunks // s)
    se = -(-nchunks // cps)
    ok = (npp <= MAX_NPP) & (4 * npp * 64 + nb * cps * 32 * 4 <= LDS_MAX)
    blocks = tiles * se
    full, rest = blocks // 256, blocks % 256
    tb = cps * 6000 + 4000
    tail = np.where(rest > 0, tb, 0)
    subq = np.ones_like(blocks)
    for q, pct in ((2, SUB2_PCT), (4, SUB4_PCT)):
        take = (rest > 0) & (q * rest <= 256) & (tb * pct // 100 < tail)
        tail, subq = np.where(take, tb * pct // 100, tail), np.where(take, q, subq)
    cost = full * tb + tail + blocks * 40 + np.where(tw < 8, 8 - tw, 0)
    cost = cost + np.where(se > 1, (float(N * OH * OW * Co) * 4.0 * (2 * se + 1) / 4000.0).astype(np.int64) + 3000, 0)
    if not ok.any():
        return None
    i, j = divmod(int(np.argmin(np.where(ok, cost, np.iinfo(np.int64).max))), s.shape[1])
    P = case(N=N, IH=IH, IW=IW, Ci=Ci, Co=Co, OH=OH, OW=OW, nchunks=nchunks, ncot=ncot, TW=int(tw[i, 0]), TH=int(th[i, 0]),
             NB=int(nb[i, 0]), cps=int(cps[0, j]), nsplit=int(se[0, j]), subq=int(subq[i, j]))
    P.ntx, P.nty, P.ntn = cdiv(GW, P.TW), cdiv(GH, P.TH), cdiv(N, P.NB)
    P.tiles = P.ntx * P.nty * P.ntn * ncot
    P.items = P.tiles * P.nsplit
    P.nfull = P.items // 256 * 256 if P.subq > 1 else P.items
    P.PH = P.TH + 1
    position_map(P)
    P.lds = lds_bytes(P.NPP, P.NB, P.cps)
    P.ws_floats = P.nsplit * N * OH * OW * Co if P.nsplit > 1 else 0
    return P


def lds_bytes(npp, nb, cps):
    return 4 * npp * 64 + nb * cps * 32 * 4 + 128


LANE_A, LANE_B = (0, 1, 2, 3, 12, 13, 14, 15), (4, 5, 6, 7, 8, 9, 10, 11)


def position_map(P):
    """ct2_position_map: P.map (128 entries, bit 7 = unused slot), P.PW, P.NPP, P.kind ('perm' / 'identity'), P.pad."""
    npos, tpos = P.TW * P.TH * P.NB, P.TW * P.TH
    m = [i if i < npos else 128 | (npos - 1) for i in range(128)]
    P.PW, P.kind, P.pad = P.TW + 1, 'identity', 0
    for pad in range(4):
        PW = P.TW + 1 + pad
        npp = P.NB * P.PH * PW
        if npp > MAX_NPP or lds_bytes(npp, P.NB, P.cps) > LDS_MAX:
            break
        cls = [[] for _ in range(8)]
        for pos in range(npos):
            nbi, rem = divmod(pos, tpos)
            ty, tx = divmod(rem, P.TW)
            cls[((nbi * P.PH + ty + 1) * PW + tx + 1) & 7].append(pos)
        if max(len(c) for c in cls) > 16:
            continue
        for s in range(16):
            lanes = LANE_B if s & 1 else LANE_A
            have = [c[s] for c in cls if s < len(c)]
            for r in range(8):      # a missing residue re-reads a pixel of its own set
                m[(s >> 1) * 16 + lanes[r]] = cls[r][s] if s < len(cls[r]) else 128 | (have[0] if have else 0)
        P.PW, P.kind, P.pad = PW, 'perm', pad
        break
    P.NPP = P.NB * P.PH * P.PW
    P.map = m


def xcd_remap(bid, nwg):
    q, r, xcd = nwg >> 3, nwg & 7, bid & 7
    return np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + (bid >> 3)


def launches_of(items, nfull, subq):
    """convt2_run: (first work item, blocks, NJ) of each launch."""
    out = [(0, nfull, 8)] if nfull > 0 else []
    if subq > 1 and items > nfull:
        out.append((nfull, (items - nfull) * subq, 8 // subq))
    return out


def covered_once(items, nfull, subq):
    """The block -> (work item, fragment columns) decode of convt2_kernel over both launches: every pair exactly once."""
    hits = np.zeros(items * 8, dtype=np.int64)
    for item0, nwg, nj in launches_of(items, nfull, subq):
        r = xcd_remap(np.arange(nwg, dtype=np.int64), nwg)
        lid, jbase = item0 + r // (8 // nj), (r % (8 // nj)) * nj
        if int(lid.min()) < 0 or int(lid.max()) >= items:
            return False
        for j in range(nj):
            np.add.at(hits, lid * 8 + jbase + j, 1)
    return bool((hits == 1).all())


def form_of(P, split, pk, osc, amax):
    ls = launches_of(P.items, P.nfull, P.subq)
    red = 'nored' if P.nsplit == 1 else f'red<{"osc" if osc else "noosc"},{"amax" if amax else "noamax"}>'
    return (f'ct2<s{split},pk{int(pk)}>/' + '+'.join(f'NJ{nj}' for _, _, nj in ls) + f'/t{P.TW}x{P.TH}x{P.NB}/pw{P.PW}-{P.kind}'
            f'/s{P.nsplit}x{P.cps}/{red}')


def geom(c):
    return (c.N, c.IH, c.IW, c.Ci, c.Co, 2 * c.IH + c.oh, 2 * c.IW + c.ow)


def replay(c):
    """convt2_run for one case: rc and the gate's name, or the form."""
    r = case(rc=0, why=None, form=None, P=None)

    def refuse(why):
        r.rc, r.why = EINVAL, why
        return r
    if c.pk and (c.bad == 'hdr-null' or c.Ci & 31):
        return refuse('split-entry')
    if c.bad.startswith('null-') or c.split not in (1, 2):
        return refuse('null' if c.bad.startswith('null-') else 'split')
    if c.bad.startswith('align-'):
        return refuse('align')
    r.P = ct2_plan(*geom(c))
    if r.P is None:
        return refuse('shape')
    if r.P.nsplit > 1 and c.bad in ('ws-null', 'ws-misaligned'):
        return refuse('workspace')
    assert r.P.lds <= LDS_MAX and r.P.items * r.P.subq <= 0x7fffffff        # (gates of convt2_run the plan itself already keeps)
    r.form = form_of(r.P, c.split, c.pk, c.osc, c.amax)
    return r


def want_of(c):
    r = replay(c)
    return r, (r.form if r.rc == 0 else f'EINVAL:{r.why}')


def lib_plan(g):
    from rick_amd._lib import lib
    plan, pm, pitch = (ctypes.c_int * 8)(), (ctypes.c_ubyte * 128)(), ctypes.c_int(0)
    rc = lib.rick_convt2_plan(*g, plan)
    rc2 = lib.rick_convt2_posmap(*g, pm, ctypes.byref(pitch))
    assert rc == rc2
    return rc, list(plan), list(pm), pitch.value, lib.rick_convt2_workspace_bytes(*g)


# ------------------------------------------------------------------------------------------------------- case table
def C(N, IH, IW, Ci, Co, want, split=2, pk=0, isc=0, osc=0, amax=0, oh=0, ow=0, amp=4, bad=''):
    """One case; `want` is the literal it must reach.  pk: the split-image entry (x is a split image; iscale, if any, is folded
    into it); isc / osc: iscale / oscale given; amax: an amax word (split entry only); oh / ow: OH = 2 IH + oh, OW = 2 IW + ow;
    amp: integer amplitude of the exact modes; bad: what makes the call invalid (refusals)."""
    tag = f'N{N}-{IH}x{IW}-Ci{Ci}-Co{Co}-o{oh}{ow}' + (f'-split{split}' if split != 2 else '') + ('-pk' if pk else '') + \
          ('-isc' if isc else '') + ('-osc' if osc else '') + ('-amax' if amax else '') + (f'-bad:{bad}' if bad else '')
    return case(id=want + '-' + tag, want=want, N=N, IH=IH, IW=IW, Ci=Ci, Co=Co, split=split, pk=pk, isc=isc, osc=osc, amax=amax,
                oh=oh, ow=ow, amp=amp, bad=bad)


CASES = [
    # one sub-block launch of four blocks, two columns each: the smallest grids
    C(1, 1, 1, 4, 4, 'ct2<s2,pk0>/NJ2/t2x2x1/pw3-perm/s1x1/nored', isc=1),
    C(1, 1, 1, 4, 4, 'ct2<s1,pk0>/NJ2/t2x2x1/pw3-perm/s1x1/nored', split=1, osc=1, oh=1),
    C(1, 1, 1, 32, 4, 'ct2<s2,pk1>/NJ2/t2x2x1/pw3-perm/s1x1/nored', pk=1, amax=1, ow=1),
    C(1, 1, 1, 64, 4, 'ct2<s2,pk0>/NJ2/t2x2x1/pw3-perm/s2x1/red<osc,noamax>', osc=1),
    C(1, 1, 1, 64, 4, 'ct2<s2,pk1>/NJ2/t2x2x1/pw3-perm/s2x1/red<osc,amax>', pk=1, amax=1, osc=1, oh=1, ow=1),
    C(1, 1, 1, 64, 4, 'ct2<s2,pk1>/NJ2/t2x2x1/pw3-perm/s2x1/red<noosc,noamax>', pk=1),
    C(2, 3, 1, 32, 4, 'ct2<s2,pk1>/NJ2/t2x4x2/pw3-perm/s1x1/nored', pk=1, isc=1),
    C(1, 2, 1, 36, 4, 'ct2<s2,pk0>/NJ2/t2x3x1/pw3-perm/s2x1/red<osc,noamax>', isc=1, osc=1, oh=1),
    C(1, 2, 1, 36, 4, 'ct2<s1,pk0>/NJ2/t2x3x1/pw3-perm/s2x1/red<noosc,noamax>', split=1, oh=1),
    # several tiles in y / n / x with ragged last ones, masked image slots, the three map kinds
    C(11, 4, 1, 4, 4, 'ct2<s2,pk0>/NJ2/t2x3x11/pw3-perm/s1x1/nored', osc=1, oh=1),
    C(12, 2, 4, 8, 4, 'ct2<s2,pk0>/NJ2/t5x3x8/pw6-identity/s1x1/nored', isc=1, osc=1),
    C(12, 2, 4, 32, 4, 'ct2<s2,pk1>/NJ2/t5x3x8/pw6-identity/s1x1/nored', pk=1, amax=1),
    C(5, 1, 12, 32, 4, 'ct2<s1,pk0>/NJ2/t8x2x5/pw9-perm/s1x1/nored', split=1, isc=1, ow=1),
    C(9, 2, 2, 4, 4, 'ct2<s2,pk0>/NJ2/t3x3x9/pw5-perm/s1x1/nored', isc=1),
    C(2, 7, 10, 8, 4, 'ct2<s2,pk0>/NJ2/t8x8x2/pw9-perm/s1x1/nored', ow=1),
    C(1, 4, 2, 544, 4, 'ct2<s2,pk0>/NJ2/t3x5x1/pw4-perm/s9x2/red<noosc,noamax>', oh=1, amp=1),
    # the co tile: ragged, two and three of them, four waves masked
    C(1, 2, 1, 32, 132, 'ct2<s2,pk1>/NJ2/t2x3x1/pw3-perm/s1x1/nored', pk=1, osc=1, amax=1, oh=1),
    C(2, 1, 1, 8, 68, 'ct2<s2,pk0>/NJ2/t2x2x2/pw3-perm/s1x1/nored', osc=1, oh=1, ow=1),
    C(1, 1, 4, 8, 128, 'ct2<s1,pk0>/NJ2/t5x2x1/pw6-perm/s1x1/nored', split=1, osc=1),
    C(3, 1, 1, 8, 260, 'ct2<s2,pk0>/NJ2/t2x2x3/pw3-perm/s1x1/nored', isc=1, osc=1),
    # 65 ... 128 work items: one launch of two blocks per item
    C(13, 12, 40, 4, 4, 'ct2<s2,pk0>/NJ4/t9x13x1/pw11-perm/s1x1/nored', isc=1, osc=1),
    C(13, 12, 40, 4, 4, 'ct2<s1,pk0>/NJ4/t9x13x1/pw11-perm/s1x1/nored', split=1),
    C(13, 12, 40, 32, 4, 'ct2<s2,pk1>/NJ4/t9x13x1/pw11-perm/s1x1/nored', pk=1, amax=1),
    C(10, 39, 1, 544, 4, 'ct2<s2,pk0>/NJ4/t2x5x10/pw3-perm/s9x2/red<noosc,noamax>', oh=1, amp=1),
    C(14, 38, 1, 256, 4, 'ct2<s2,pk1>/NJ4/t2x20x3/pw3-perm/s8x1/red<osc,amax>', pk=1, osc=1, amax=1, oh=1, amp=1),
    # 129 ... 256: whole-tile blocks only
    C(11, 33, 36, 4, 4, 'ct2<s2,pk0>/NJ8/t3x7x6/pw4-identity/s1x1/nored', osc=1),
    C(11, 33, 36, 4, 4, 'ct2<s1,pk0>/NJ8/t3x7x6/pw4-identity/s1x1/nored', split=1, isc=1, oh=1, ow=1),
    C(11, 33, 36, 32, 4, 'ct2<s2,pk1>/NJ8/t3x7x6/pw4-identity/s1x1/nored', pk=1, amax=1, osc=1, ow=1),
    C(16, 12, 10, 1024, 4, 'ct2<s2,pk0>/NJ8/t11x5x2/pw12-perm/s8x4/red<noosc,noamax>', oh=1, ow=1, amp=1),
    C(11, 35, 10, 512, 4, 'ct2<s2,pk1>/NJ8/t11x9x1/pw12-perm/s4x4/red<noosc,amax>', pk=1, amax=1, amp=1),
    # a full round of whole-tile blocks, then the rest as four / two blocks per item
    C(13, 45, 48, 4, 4, 'ct2<s2,pk0>/NJ8+NJ2/t10x12x1/pw11-perm/s1x1/nored', isc=1),
    C(13, 45, 48, 4, 4, 'ct2<s1,pk0>/NJ8+NJ2/t10x12x1/pw11-perm/s1x1/nored', split=1, osc=1, ow=1),
    C(13, 45, 48, 32, 4, 'ct2<s2,pk1>/NJ8+NJ2/t10x12x1/pw11-perm/s1x1/nored', pk=1, amax=1, oh=1),
    C(13, 45, 25, 512, 4, 'ct2<s2,pk0>/NJ8+NJ2/t9x7x2/pw11-perm/s2x8/red<noosc,noamax>', oh=1, ow=1, amp=1),
    C(14, 36, 72, 4, 4, 'ct2<s2,pk0>/NJ8+NJ4/t25x5x1/pw27-perm/s1x1/nored'),
    C(14, 36, 72, 4, 4, 'ct2<s1,pk0>/NJ8+NJ4/t25x5x1/pw27-perm/s1x1/nored', split=1, isc=1, osc=1, oh=1),
    C(14, 36, 72, 32, 4, 'ct2<s2,pk1>/NJ8+NJ4/t25x5x1/pw27-perm/s1x1/nored', pk=1),
    C(16, 12, 48, 1024, 4, 'ct2<s2,pk0>/NJ8+NJ4/t9x7x2/pw11-perm/s4x8/red<noosc,noamax>', ow=1, amp=1),
]
# refused on the host before anything is launched: the output keeps every sentinel
GATES = [
    C(2, 4, 4, 6, 8, 'EINVAL:shape'),
    C(2, 4, 4, 8, 6, 'EINVAL:shape'),
    C(2, 4, 4, 8, 8, 'EINVAL:shape', oh=-1),
    C(2, 4, 4, 8, 8, 'EINVAL:shape', oh=2),
    C(2, 4, 4, 8, 8, 'EINVAL:shape', ow=-1),
    C(2, 4, 4, 8, 8, 'EINVAL:shape', ow=2),
    C(2, 4, 4, 8, 8, 'EINVAL:split', split=0),
    C(2, 4, 4, 8, 8, 'EINVAL:split', split=3),
    C(2, 4, 4, 8, 8, 'EINVAL:align', bad='align-x'),
    C(2, 4, 4, 8, 8, 'EINVAL:align', bad='align-w'),
    C(2, 4, 4, 8, 8, 'EINVAL:align', bad='align-out'),
    C(2, 4, 4, 8, 8, 'EINVAL:align', bad='align-isc', isc=1),
    C(2, 4, 4, 8, 8, 'EINVAL:align', bad='align-osc', osc=1),
    C(2, 4, 4, 8, 8, 'EINVAL:null', bad='null-x'),
    C(2, 4, 4, 8, 8, 'EINVAL:null', bad='null-w'),
    C(2, 4, 4, 8, 8, 'EINVAL:null', bad='null-out'),
    C(1, 1, 1, 64, 4, 'EINVAL:workspace', bad='ws-null'),
    C(1, 1, 1, 64, 4, 'EINVAL:workspace', bad='ws-misaligned'),
    C(2, 4, 4, 48, 8, 'EINVAL:split-entry', pk=1),
    C(2, 4, 4, 32, 8, 'EINVAL:split-entry', pk=1, bad='hdr-null'),
]
REQUIRED_GATES = {'shape', 'split', 'align', 'null', 'workspace', 'split-entry'}
LO_BLIND = set()              # split == 2 forms without an exact22 case (module docstring): none


def modes_of(c):
    return ('exact11', 'bound') + (('exact22x', 'exact22w') if c.split == 2 else ())


DEVICE = [(c, m) for c in CASES for m in modes_of(c)]


def params(pairs):
    return pytest.mark.parametrize('c,mode', pairs, ids=[f'{c.id}-{m}' for c, m in pairs])


# ----------------------------------------------------------------------------------------------------------- inputs
def scatter(A, B, OH, OW):
    """sum_ci B[co, ci, ky*3+kx] * A[n, iy, ix, ci] added into [n, 2*iy+ky, 2*ix+kx, co], cropped to OH x OW (fp64): the
    expression of include/rick_hip.h as it stands, with no parity classes."""
    N, IH, IW, Ci = A.shape
    full = torch.zeros(N, 2 * IH + 1, 2 * IW + 1, B.shape[0], dtype=torch.float64)
    a = A.reshape(-1, Ci)
    for ky in range(3):
        for kx in range(3):
            full[:, ky:ky + 2 * IH:2, kx:kx + 2 * IW:2] += (a @ B[:, :, ky * 3 + kx].t()).reshape(N, IH, IW, -1)
    return full[:, :OH, :OW].contiguous()


def _key(c, mode):
    return (c.N, c.IH, c.IW, c.Ci, c.Co, c.oh, c.ow, c.split, c.isc, c.osc, c.amp, mode)


@functools.lru_cache(maxsize=2)
def _inputs(key):
    N, IH, IW, Ci, Co, oh, ow, split, isc, osc, amp, mode = key
    sid = f'ct2f/{N}/{IH}x{IW}/{Ci}/{Co}/{mode}'
    exact = mode != 'bound'
    b = case(exact=exact, alpha=0.25 if exact else f32(1 / math.sqrt(2)), wscale=1.0 if exact else f32(2 ** -0.5), OH=2 * IH + oh,
             OW=2 * IW + ow, K=4 * Ci, split=split)
    xs, ws = (N, IH, IW, Ci), (Co, Ci, 9)
    if mode == 'bound':
        b.x, b.w = synth_tensor(sid + '/x', xs), synth_tensor(sid + '/w', ws)
    elif mode == 'exact11':
        b.x, b.w = ints(sid + '/x', xs, amp), ints(sid + '/w', ws, amp)
    elif mode == 'exact22x':
        b.x, b.w = fine(sid + '/x', xs), ints(sid + '/w', ws, min(amp, 2))
    else:
        b.x, b.w = ints(sid + '/x', xs, min(amp, 2)), fine(sid + '/w', ws)
    b.isc = scales(sid + '/isc', (N, Ci), mode) if isc else None
    b.osc = scales(sid + '/osc', (N, Co), mode) if osc else None
    b.X = b.x.double() * (b.isc.double()[:, None, None, :] if isc else 1.0)
    b.W = b.w.double() * float(b.wscale)
    b.unit = b.alpha * (0.5 if isc else 1.0) * (0.5 if osc else 1.0) * (1.0 if mode in ('exact11', 'bound') else 2.0 ** -10)
    if exact:
        # the premises of the exact modes, from an upper bound of sum |terms| that needs no contraction; |hi| + |lo| of a
        # fine() value exceeds |v| by less than 2**-9 of it
        omax = float(b.osc.max()) if osc else 1.0
        sub = float(scatter(b.X.abs(), torch.ones(1, Ci, 9, dtype=torch.float64), b.OH, b.OW).max()) * float(b.W.abs().max()) * b.alpha * omax
        sub *= 1.0 if mode == 'exact11' else 1 + 2.0 ** -9
        assert sub / b.unit < 2 ** 24, f'{sid}: sum |terms| <= {sub / b.unit} units: not exact in fp32'
        for name, v in (('x', b.X), ('w', b.W)):
            lim = 11 if mode == 'exact11' or name != mode[-1] else 12
            q = v.abs()
            assert bool((q * 2.0 ** 11 == (q * 2.0 ** 11).round()).all()) and float(q.max()) / float(q[q > 0].min()) <= 16, name
            assert lim == 12 or bool((q.float().half().double() == q).all()), f'{name}: more than 11 bits'
    for name, v, Cn in (('x', b.x, Ci), ('w', b.w.permute(0, 2, 1), Ci), ('w', b.w.permute(1, 2, 0), Co)):
        assert float(v.min()) < 0 < float(v.max()), f'{name}: one sign only'
        if 32 <= v.numel() // Cn <= 1 << 16:             # (fewer rows of +-1 cannot tell 544 channels apart)
            assert torch.unique(v.reshape(-1, Cn).t(), dim=0).shape[0] == Cn, f'{name}: two equal channels'
    assert N == 1 or IH * IW * Ci < 32 or torch.unique(b.x.reshape(N, -1), dim=0).shape[0] == N, 'x: two equal images'
    return b


def inputs(c, mode):
    return _inputs(_key(c, mode))


def term_counts(IH, IW, Ci, OH, OW):
    """Terms of every output element: Ci x (taps that reach it) -> [1, OH, OW, 1]."""
    one = torch.ones(1, IH, IW, 1, dtype=torch.float64)
    return scatter(one, torch.ones(1, 1, 9, dtype=torch.float64), OH, OW) * Ci


@functools.lru_cache(maxsize=2)
def _reference(key):
    """The fp64 result on [N, OH, OW, Co], every element's own K, and in `bound` the sums the bound needs."""
    b = _inputs(key)
    N, IH, IW, Ci, Co = key[:5]
    mode = key[-1]
    osc = b.osc.double()[:, None, None, :] if b.osc is not None else 1.0
    r = case(ref=b.alpha * osc * scatter(b.X, b.W, b.OH, b.OW), K=term_counts(IH, IW, Ci, b.OH, b.OW))
    # interior elements carry Ci x {4, 2, 2, 1} terms by parity class, border elements fewer, none zero
    want = torch.tensor([[4.0, 2.0], [2.0, 1.0]])[torch.arange(b.OH)[:, None] % 2, torch.arange(b.OW)[None, :] % 2] * Ci
    k2 = r.K[0, :, :, 0]
    assert bool((k2 <= want).all()) and bool((k2 >= Ci).all()) and torch.equal(k2[1:2 * IH - 1, 1:2 * IW - 1], want[1:2 * IH - 1, 1:2 * IW - 1])
    assert tuple(r.ref.shape) == (N, b.OH, b.OW, Co)
    if mode == 'bound':
        P = ct2_plan(N, IH, IW, Ci, Co, b.OH, b.OW)
        oa = b.alpha * (osc if b.osc is None else osc.abs())
        r.S = oa * scatter(b.X.abs(), b.W.abs(), b.OH, b.OW)
        sw = scatter(torch.ones(1, IH, IW, Ci, dtype=torch.float64), b.W.abs(), b.OH, b.OW)            # [1, OH, OW, Co]
        sx = scatter(b.X.abs(), torch.ones(1, Ci, 9, dtype=torch.float64), b.OH, b.OW)                 # [N, OH, OW, 1]
        wn = oa * (float(b.X.abs().max()) * sw + float(b.W.abs().max()) * sx)
        r.rep = rep_of(b.split)
        r.win = 2.0 ** -27 * wn
        r.bnd = bound_terms(r.S, wn, 0.0, r.K, R_ROUND, r.rep) + (P.nsplit if P.nsplit > 1 else 0) * 2.0 ** -24 * r.S + 2.0 ** -23 * r.ref.abs()
    if b.exact:
        assert torch.equal(r.ref.float().double(), r.ref) and not bool((r.ref == SENT).any())
    assert float(r.ref.min()) < 0 < float(r.ref.max())
    return r


def emulate(b, lo=True):
    """The documented split on the CPU with one exponent per operand: products hi*hi + hi*lo + lo*hi (no lo*lo), summed in fp64."""
    xh, xl, ux = split_halves(b.X, lo and b.split == 2)
    wh, wl, uw = split_halves(b.W, lo and b.split == 2)
    osc = b.osc.double()[:, None, None, :] if b.osc is not None else 1.0
    return b.alpha * osc * ux * uw * (scatter(xh, wh, b.OH, b.OW) + scatter(xh, wl, b.OH, b.OW) + scatter(xl, wh, b.OH, b.OW))


# ---------------------------------------------------------------------------------------------------- host-only tests
def _feat(c, P):
    """The coverage items one case reaches, named from the replay (REQUIRED lists what the table must reach together)."""
    ls = launches_of(P.items, P.nfull, P.subq)
    inst = {f'ct2<s{c.split},pk{c.pk}>/NJ{nj}' for _, _, nj in ls}
    shape = '+'.join(f'NJ{nj}' for _, _, nj in ls)
    GH, GW = c.IH + 1, c.IW + 1
    f = set(inst) | {'launch:' + shape + ('/split-K' if P.nsplit > 1 else '')}
    f.add(f'map:{P.kind}' + (f'/pad{P.pad}' if P.kind == 'perm' else '') + ('+unused' if P.TW * P.TH * P.NB < 128 else ''))
    f |= {'NB=1' if P.NB == 1 else 'NB>1', 'N%NB' if c.N % P.NB else '', 'ntx>1' if P.ntx > 1 else '', 'nty>1' if P.nty > 1 else '',
          'ntn>1' if P.ntn > 1 else '', 'ncot>1' if P.ncot > 1 else '', 'ragged x' if GW % P.TW else '', 'ragged y' if GH % P.TH else '',
          'cps=1' if P.cps == 1 else 'cps>1', 'nchunks%cps' if P.nchunks % P.cps else '',
          'cps>1, short last split' if P.cps > 1 and P.nchunks % P.cps and P.nsplit > 1 else '',
          'Ci%32' if c.Ci % 32 else '', 'Ci%32, split-K' if c.Ci % 32 and P.nsplit > 1 else '',
          'Co=4' if c.Co == 4 else '', 'Co<=64' if c.Co <= 64 else '', 'Co 65..127' if 65 <= c.Co <= 127 else '', 'Co=128' if c.Co == 128 else '',
          'Co=132' if c.Co == 132 else '', 'Co>256' if c.Co > 256 else '',
          f'OH=2IH+{c.oh}', f'OW=2IW+{c.ow}', 'OH, OW mixed' if c.oh != c.ow else '',
          'iscale' if c.isc and not c.pk else 'no iscale', 'oscale' if c.osc else 'no oscale',
          'oscale through reduce' if c.osc and P.nsplit > 1 else '', 'oscale on the direct store' if c.osc and P.nsplit == 1 else '',
          'sub-block grid % 8' if len(ls) and ls[-1][2] < 8 and ls[-1][1] % 8 else ''}
    if c.pk:
        f.add(('amax' if c.amax else 'no amax') + (', one split' if P.nsplit == 1 else ', several splits'))
    if c.split == 2:
        f |= {'e22:' + k for k in inst}
    f.discard('')
    return f


_INST = {f'ct2<s{s},pk{pk}>/NJ{nj}' for s, pk in ((1, 0), (2, 0), (2, 1)) for nj in (8, 4, 2)}
REQUIRED = (
    _INST | {'e22:' + k for k in _INST if k.startswith('ct2<s2')}
    | {'launch:' + s + k for s in ('NJ8', 'NJ4', 'NJ2', 'NJ8+NJ4', 'NJ8+NJ2') for k in ('', '/split-K')}
    | {'map:perm/pad0', 'map:perm/pad0+unused', 'map:perm/pad1+unused', 'map:identity+unused'}
    | {'NB=1', 'NB>1', 'N%NB', 'ntx>1', 'nty>1', 'ntn>1', 'ncot>1', 'ragged x', 'ragged y', 'cps=1', 'cps>1', 'nchunks%cps',
       'cps>1, short last split', 'Ci%32', 'Ci%32, split-K', 'Co=4', 'Co<=64', 'Co 65..127', 'Co=128', 'Co=132', 'Co>256',
       'OH=2IH+0', 'OH=2IH+1', 'OW=2IW+0', 'OW=2IW+1', 'OH, OW mixed', 'iscale', 'no iscale', 'oscale', 'no oscale',
       'oscale through reduce', 'oscale on the direct store', 'sub-block grid % 8'}
    | {f'{a}, {s}' for a in ('amax', 'no amax') for s in ('one split', 'several splits')})


def sweep_geometries(n=3000):
    rnd = random.Random(18)
    for _ in range(n):
        N, IH, IW = rnd.randint(1, 16), rnd.randint(1, 48), rnd.randint(1, 48)
        Ci = rnd.choice([4, 8, 12, 32, 36, 64, 96, 100, 128, 160, 256, 512, 544, 1024])
        Co = rnd.choice([4, 8, 64, 68, 100, 128, 132, 256, 260, 512])
        yield (N, IH, IW, Ci, Co, 2 * IH + rnd.randint(0, 1), 2 * IW + rnd.randint(0, 1))


def held_to_library(g, what):
    """The replayed plan and map are the library's; the invariants, from the library's output alone."""
    P = ct2_plan(*g)
    rc, plan, pm, pitch, ws = lib_plan(g)
    if P is None:
        assert rc == EINVAL and ws == -1, what
        return None
    assert rc == 0, what
    assert plan == [P.TW, P.TH, P.NB, P.tiles, P.nsplit, P.cps, P.nfull, P.subq], f'{what}: rick_convt2_plan says {plan}'
    assert pm == P.map and pitch == P.PW, f'{what}: rick_convt2_posmap differs from the replay (pitch {pitch} / {P.PW})'
    assert ws == P.ws_floats * 4, what
    N, IH, IW, Ci, Co, OH, OW = g
    tw, th, nb, tiles, nsplit, cps, nfull, subq = plan
    npos = tw * th * nb
    assert 1 <= npos <= 128 and nb <= N and tiles == cdiv(IW + 1, tw) * cdiv(IH + 1, th) * cdiv(N, nb) * cdiv(Co, 128), what
    assert sorted(e for e in pm if e < 128) == list(range(npos)), f'{what}: the live entries are no permutation of the tile'
    assert all(e & 127 < npos for e in pm), f'{what}: an unused slot carries a position outside the tile'
    assert tw + 1 <= pitch <= tw + 4 and nb * (th + 1) * pitch <= MAX_NPP, what
    assert lds_bytes(nb * (th + 1) * pitch, nb, cps) <= LDS_MAX, what
    assert 1 <= nsplit <= 16 and nsplit == cdiv(cdiv(Ci, 32), cps), what
    items = tiles * nsplit
    assert subq in (1, 2, 4) and (nfull == items if subq == 1 else nfull == items // 256 * 256 and 0 < (items - nfull) * subq <= 256), what
    assert covered_once(items, nfull, subq), f'{what}: the two launches do not cover every (work item, fragment column) once'
    return P


def test_case_ids_replay_and_library_agree():
    """No device.  Every case's literal `want` is what the replayed planner and launcher pick; the replay is the library's own
    plan, position map and workspace size on every case and on the sweep; the map's invariants hold on the sweep; the table
    reaches the whole coverage list and every gate; the size caps hold."""
    from rick_amd._lib import lib
    assert len({c.id for c in CASES + GATES}) == len(CASES + GATES)
    reached, gates = set(), set()
    for c in CASES + GATES:
        r, want = want_of(c)
        assert want == c.want, f'{c.id}: the replay reaches {want}'
        P = held_to_library(geom(c), c.id)
        if c in CASES:
            assert r.rc == 0 and not c.bad and P is r.P, c.id
            assert not c.amax or c.pk, f'{c.id}: only the split entry takes an amax word'
            assert not c.pk or c.split == 2
            reached |= _feat(c, P)
            assert c.N * (2 * c.IH + c.oh) * (2 * c.IW + c.ow) * c.Co * (1 + (P.nsplit if P.nsplit > 1 else 0)) <= MAX_OUT_FLOATS, c.id
            assert c.N * c.IH * c.IW * c.Ci * c.Co * 9 <= MAX_MACS, c.id
        else:
            assert r.rc == EINVAL, c.id
            gates.add(r.why)
            if r.why == 'shape':
                assert lib.rick_convt2_workspace_bytes(*geom(c)) == -1, c.id
    assert not REQUIRED - reached, f'not reached: {sorted(REQUIRED - reached)}'
    assert not REQUIRED_GATES - gates, f'gates not reached: {sorted(REQUIRED_GATES - gates)}'
    assert len(DEVICE) + len(GATES) <= 160
    kinds = {}
    for g in sweep_geometries():
        P = held_to_library(g, str(g))
        if P is not None:
            k = f'{P.kind}/pad{P.pad}' + ('+unused' if P.TW * P.TH * P.NB < 128 else '')
            kinds[k] = kinds.get(k, 0) + 1
    print(f'map kinds of the sweep: {sorted(kinds.items())}')
    assert {'perm/pad0', 'perm/pad0+unused', 'perm/pad1+unused', 'identity/pad0+unused'} <= set(kinds)
    assert not any('pad2' in k or 'pad3' in k for k in kinds), 'the sweep reaches a pad the case table has no case for'


def test_exact_inputs_fit_and_the_bound_sees_a_lost_lo_half_where_it_can():
    """No device.  Every exact-mode builder passes its own assertions (sum |terms| < 2**24 units from an upper bound, operands of
    11 / 12 bits inside the 32x window, distinct channels and images, mixed signs).  On the split == 2 cases with K <= 160 the
    CPU emulation of the documented split stays inside the representation and below-window parts of the bound alone (one exponent
    for a whole tensor leaves more values below the 32x window than a block's does), and an emulation without the lo halves
    leaves the whole bound: the bound can tell a lost half.  Every split == 2 case beyond that runs exact22."""
    for c, mode in DEVICE:
        if mode != 'bound':
            inputs(c, mode)
    done = 0
    for c in CASES:
        if 4 * c.Ci > 160:
            assert c.split == 1 or 'exact22x' in modes_of(c) or c.want in LO_BLIND, c.id
            continue
        b, r = inputs(c, 'bound'), _reference(_key(c, 'bound'))
        err = (emulate(b) - r.ref).abs()
        part = r.rep * r.S + r.win
        assert bool((err <= part).all()), f'{c.id}: emulated split {float((err / part).max()):.3f} x the representation and window parts'
        if c.split == 2:
            worst = float(((emulate(b, lo=False) - r.ref).abs() / r.bnd).max())
            assert worst > 1, f'{c.id}: the bound does not see a lost lo half ({worst:.3f})'
            done += 1
    assert done >= 8 and not LO_BLIND


# ----------------------------------------------------------------------------------------------------- device helpers
def pack_weight(b, split):
    from rick_amd._lib import lib
    Co, Ci = b.w.shape[0], b.w.shape[1]
    src, pk = fenced(b.w), Fenced(lib.rick_conv_packed_bytes(Co, Ci, 9) // 4)
    assert lib.rick_conv_pack_weight(p(src), Ci * 9, 9, 1, Co, Ci, 9, float(b.wscale), split, p(pk), stream()) == 0
    torch.cuda.synchronize()
    assert nan_fence_ok(pk), 'rick_conv_pack_weight wrote outside the packed image'
    return pk


def upload(c, b, bad=''):
    """Every operand of the call as a fenced view; `bad` misaligns one or takes it away."""
    o = case()
    off = lambda name: 1 if bad == 'align-' + name else 0
    o.w = pack_weight(b, c.split if c.split in (1, 2) else 2)
    if off('w'):
        o.w = case(v=o.w.buf[65:])
    o.x, o.hdr = split_image(b.X.float()) if c.pk else (fenced(b.x, off('x')), None)
    o.x32 = fenced(b.X.float()) if c.pk else None          # the same values for the fp32 entry
    o.isc = None if c.pk else fenced(b.isc, off('isc'))
    o.osc = fenced(b.osc, off('osc'))
    if bad == 'hdr-null':
        o.hdr = None
    if bad in ('null-x', 'null-w'):
        setattr(o, bad[-1], None)
    return o


def run_once(c, b, o, P, ws_null=False, bad='', fp32_twin=False):
    """One launch into fresh guarded buffers -> (rc, the buffers), the bands checked."""
    from rick_amd._lib import lib
    g = geom(c)
    got = case(out=Guarded(g[0] * g[5] * g[6] * g[4]), ws=Guarded(max(P.ws_floats if P else 0, 4)),
               word=Guarded(AMAX_FLOATS, torch.zeros(AMAX_FLOATS)) if c.amax and not fp32_twin else None)
    wsp = None if ws_null or bad == 'ws-null' else got.ws.buf[got.ws.lo + 1:].data_ptr() if bad == 'ws-misaligned' else p(got.ws)
    outp = None if bad == 'null-out' else got.out.buf[got.out.lo + 1:].data_ptr() if bad == 'align-out' else p(got.out)
    if c.pk and not fp32_twin:
        got.rc = lib.rick_convt2_split_f32(p(o.x), p(o.hdr), p(o.w), outp, p(o.osc), *g, float(b.alpha), p(got.word), wsp, stream())
    else:
        got.rc = lib.rick_convt2_f32(p(o.x32 if fp32_twin else o.x), p(o.w), outp, p(o.isc), p(o.osc), *g, c.split, float(b.alpha), wsp, stream())
    torch.cuda.synchronize()
    for what, gd in (('out', got.out), ('workspace', got.ws), ('amax word', got.word)):
        if gd is not None:
            gd.assert_bands(f'{c.id} {what}')
    return got


def check_result(c, mode, b, P, rf, got):
    dev = got.out.v.detach().cpu().reshape(rf.ref.shape)
    left = dev.view(torch.int32) == torch.tensor(SENT).view(torch.int32)
    assert not bool(left.any()), f'{c.id}: {int(left.sum())} output elements were never written, first at {tuple(left.nonzero()[0].tolist())}'
    if mode != 'bound':
        exp = rf.ref.float()
        wrong = dev != exp
        if bool(wrong.any()):
            at = wrong.nonzero()
            d = (dev.double() - rf.ref)[wrong].abs() / b.unit
            raise AssertionError(f'{c.id}: {int(wrong.sum())} of {wrong.numel()} elements differ (n {sorted(set(at[:, 0].tolist()))[:8]}.., rows '
                                 f'{sorted(set(at[:, 1].tolist()))[:8]}.., cols {sorted(set(at[:, 2].tolist()))[:8]}.., co '
                                 f'{sorted(set(at[:, 3].tolist()))[:8]}..), by {float(d.min())} .. {float(d.max())} units; first at '
                                 f'{tuple(at[0].tolist())}: {float(dev[wrong][0])} != {float(exp[wrong][0])}')
    else:
        err = (dev.double() - rf.ref).abs()
        worst = float((err / rf.bnd.clamp_min(1e-300)).max())
        print(f'{c.id}: max |err| / bound = {worst:.4f} (K = {b.K}, nsplit = {P.nsplit})')
        assert bool((err <= rf.bnd).all()), f'{c.id}: |err| up to {worst:.3f} x the a-priori bound'
    if c.amax:
        amax_word_check(got.word.v.detach().cpu(), float(dev.abs().max()), c.id)


# -------------------------------------------------------------------------------------------------------- GPU tests
@gpu
@params(DEVICE)
def test_convt2_forms(c, mode):
    r, want = want_of(c)
    assert want == c.want and r.rc == 0
    P = r.P
    b, rf = inputs(c, mode), _reference(_key(c, mode))
    sat0 = sat_count()
    o = upload(c, b)
    # the second launch: `bound` must repeat its bits; with one split it also passes no workspace at all
    runs = [run_once(c, b, o, P, ws_null=bool(k) and P.nsplit == 1) for k in range(2 if mode == 'bound' or P.nsplit == 1 else 1)]
    assert all(g.rc == 0 for g in runs), f'{c.id}: rc = {[g.rc for g in runs]}'
    check_result(c, mode, b, P, rf, runs[0])
    if P.nsplit == 1:
        assert runs[0].ws.untouched(), f'{c.id}: one split, and the workspace was written'
    bits = lambda t: t.view(torch.int32)
    for other in runs[1:]:
        assert torch.equal(bits(runs[0].out.v), bits(other.out.v)), f'{c.id}: two launches differ'
        assert not c.amax or torch.equal(bits(runs[0].word.v), bits(other.word.v)), f'{c.id}: two launches leave different amax words'
    if c.pk and mode != 'bound':
        twin = run_once(c, b, o, P, fp32_twin=True)
        assert twin.rc == 0 and torch.equal(bits(twin.out.v), bits(runs[0].out.v)), f'{c.id}: the split entry and the fp32 entry differ on the same values'
    assert nan_fence_ok(o.w), f'{c.id}: the packed weight was written'
    assert sat_count() == sat0


@gpu
@pytest.mark.parametrize('c', GATES, ids=[c.id for c in GATES])
def test_convt2_refuses_on_the_host(c):
    """RICK_EINVAL before anything is launched: output, workspace and amax word keep every sentinel."""
    r, want = want_of(c)
    assert want == c.want and r.rc == EINVAL
    b = inputs(c, 'exact11')
    o = upload(c, b, c.bad)
    got = run_once(c, b, o, r.P, bad=c.bad)
    assert got.rc == EINVAL, f'{c.id}: rc = {got.rc}'
    assert got.out.untouched() and got.ws.untouched() and (got.word is None or bool((got.word.v == 0).all()))
