"""Every dispatch form of the fused bias / noise / LeakyReLU kernels of rick_amd/csrc/elementwise.hip — the forward
(bias_act_kernel<VEC4>), the one-pass backward (bias_act_bwd_kernel<VEC4, SPL> with its DOT form and bab_dot_reduce_kernel)
and the column-sum second stages (partial_colsum_kernel<8> / <1>, colsum_multi_kernel) — through the C ABI, against fp64
expressions written out here.  The method is that of tests/test_gpu_thin_forms.py (whose helpers this module imports):

  exact   small-integer operands, alpha = 0.25, scale = 2, noise_w = -2, mul2 = 0.5, chan_scale and the DOT divisor powers of
          two, sized so that sum |terms| < 2**24 units for every output element (asserted on the CPU before the launch): gx, gb,
          gnw, gd, every partial row and the forward output must be torch.equal to the fp64 expression cast to fp32.
  bound   standard-normal operands at the model's alpha = 0.2, scale = sqrt(2): |dev - ref64| <= (n + k) * 2**-24 * sum |terms|
          plus one ulp, n summed terms, k extra roundings per term (counted next to each builder).  Loose for the long row
          sums; the exact check carries those.

    o   = g * (ref > 0 ? 1 : alpha) * scale                                  gx
    gb  = sum_rows o                                                         per channel
    gnw = sum o * noise[(img % noise_nb), pix]                               img = row / rows_per_img, pix = row % rows_per_img
    gd[n, c] = sum_pix o * (unact(ref) - nw * noise - bias[c]) / divisor[n, c],   unact(y) = y / scale (y > 0), y / (scale alpha)

Outputs, partials, dpartials and the gradient destinations sit between sentinel bands and are pre-filled with the sentinel:
what the kernel must not write keeps it, and the partial rows of empty blocks must be written as zeros.  The launcher's
choices (blocks, rows per block, vector / scalar, column chunks, loop trips, noise path, dot_ok, bpi, colsum groups) are
replayed on the host and named in each case id; test_replay_* need no device.
"""
import ctypes
import math
import types

import pytest
import torch

from rick_amd.synth import synth_tensor
from tests.test_gpu_thin_forms import (DEV, EINVAL, MODES, SENT, U, Guarded, case, compare, dev_in, divisor_for, f32, fill, p,
                                       params, self_check, stream)

gpu = pytest.mark.gpu
AMAX_FLOATS, AMAX_STRIDE = 512, 32        # a running-maximum word: 16 slots, one per 128-byte line (include/rick_hip.h)
COLSUM_MAX = 32                           # RICK_COLSUM_MAX
EW_GRID_CAP = 256 * 16                    # ew_grid(): blocks of 256 threads, grid-stride beyond


# ------------------------------------------------------------------------------------------ host-side launcher replay
def bab_blocks(rows):
    return max(1, min(512, -(-rows // 16)))


def bab_plan(rows, C, vec):
    """bias_act_bwd_run / bias_act_bwd_kernel, replayed: blocks, rows per block, the column chunks (cg, rpb) and the set of
    (unrolled trips, remainder trips) over the thread rows of the first, the last non-empty and an empty block."""
    nb = bab_blocks(rows)
    rpblk = -(-rows // nb)
    ncol = C // (4 if vec else 1)
    chunks = [(min(256, ncol - cb), 256 // min(256, ncol - cb)) for cb in range(0, ncol, 256)]
    nonempty = -(-rows // rpblk)
    blocks = {'first': 0, 'last': nonempty - 1}
    if nonempty < nb:
        blocks['empty'] = nb - 1
    trips = {}
    for kind, b in blocks.items():
        r0, r1 = b * rpblk, min(b * rpblk + rpblk, rows)
        s = set()
        for _, rpb in chunks:
            for lane_r in range(rpb):
                r, u, m = r0 + lane_r, 0, 0
                while vec and r + 3 * rpb < r1:
                    r, u = r + 4 * rpb, u + 1
                while r < r1:
                    r, m = r + rpb, m + 1
                s.add((u, m))
        trips[kind] = s
    return types.SimpleNamespace(nb=nb, rpblk=rpblk, chunks=chunks, nonempty=nonempty, trips=trips, vec=vec)


def noise_path(N, noise_nb):
    if not noise_nb:
        return 'none'
    if noise_nb == N:
        return 'persample'                 # noise_nb * rows_per_img == rows: the index is the row
    return 'shared' if noise_nb == 1 else 'wrapped'


def noise_walk(rows, C, vec, hw, noise_nb):
    """The incremental noise index of the shared / wrapped path, replayed thread row by thread row.  Asserts that the index of
    every visited row is (img % noise_nb) * hw + pix, and returns the set of (loop, wrap-loop iterations of the step that led
    to this visit capped at 2, whether that step reset img to 0) over every visit but a thread's first."""
    plan = bab_plan(rows, C, vec)
    blks = range(plan.nonempty) if rows <= 20000 else sorted({0, 1, 2, plan.nonempty // 2, plan.nonempty - 1})
    seen = set()
    for b in blks:
        r0, r1 = b * plan.rpblk, min(b * plan.rpblk + plan.rpblk, rows)
        for _, rpb in plan.chunks:
            for lane_r in range(rpb):
                r = r0 + lane_r
                img = r // hw
                pix = r - img * hw
                img %= noise_nb
                last = None

                def visit(row, loop):
                    nonlocal img, pix, last
                    assert img * hw + pix == ((row // hw) % noise_nb) * hw + row % hw, (rows, C, hw, noise_nb, row)
                    if last is not None:
                        seen.add((loop,) + last)
                    pix += rpb
                    it, reset = 0, False
                    while pix >= hw:
                        pix -= hw
                        reset |= img + 1 == noise_nb and noise_nb > 1
                        img = 0 if img + 1 == noise_nb else img + 1
                        it += 1
                    last = (min(it, 2), reset)
                while vec and r + 3 * rpb < r1:
                    for u in range(4):
                        visit(r + u * rpb, 'U')
                    r += 4 * rpb
                while r < r1:
                    visit(r, 'R')
                    r += rpb
    return seen


def dot_ok(rows, C, hw):
    if rows <= 0 or C <= 0 or C & 3 or hw <= 0 or rows % hw:
        return 0
    nb = bab_blocks(rows)
    return int(rows % nb == 0 and hw % -(-rows // nb) == 0)


def dot_reduce_trips(bpi):
    """bab_dot_reduce_kernel: (two-way unrolled trips, remainder trips) over its 32 row groups."""
    s = set()
    for grp in range(32):
        b, u, m = grp, 0, 0
        while b + 32 < bpi:
            b, u = b + 64, u + 1
        while b < bpi:
            b, m = b + 32, m + 1
        s.add((u, m))
    return s


def colsum_plan(nb, ncols):
    """launch_colsum / partial_colsum_kernel: (CPB, G, {(four-way unrolled trips, remainder trips)} over the G row groups)."""
    cpb = 1 if ncols == 1 else 8
    G = 256 // cpb
    s = set()
    for grp in range(G):
        b, u, m = grp, 0, 0
        while b + 3 * G < nb:
            b, u = b + 4 * G, u + 1
        while b < nb:
            b, m = b + G, m + 1
        s.add((u, m))
    return cpb, G, s


def fwd_plan(n, bias, step_b, size_b, noise, n_div, hw_div, aligned=True):
    """rick_bias_act_f32: (vector?, blocks, whether a thread takes a second grid-stride trip)."""
    vec = n % 4 == 0 and (not bias or (step_b == 1 and size_b % 4 == 0)) and (not noise or (hw_div % 4 == 0 and n_div % 4 == 0)) \
        and aligned
    items = n // 4 if vec else n
    blocks = max(1, min(EW_GRID_CAP, -(-items // 256)))
    return vec, blocks, items > blocks * 256


def _trips(s):
    return '.'.join(f'u{u}r{m}' for u, m in sorted(s))


# ---------------------------------------------------------------------------------------------- backward: case tables
def _bab(N, hw, C, noise_nb=0, want='b', acc=0, og=0, oref=0, ogx=0, nopart=False, note=''):
    rows = N * hw
    vec = C % 4 == 0 and not (og or oref or ogx)
    pl = bab_plan(rows, C, vec)
    tag = (f'{"vec" if vec else "scalar"}-C{C}-N{N}x{hw}-nb{pl.nb}x{pl.rpblk}-ch{"+".join(f"{cg}x{rpb}" for cg, rpb in pl.chunks)}'
           f'-t{"|".join(k[0] + ":" + _trips(v) for k, v in pl.trips.items())}-nz.{noise_path(N, noise_nb)}{noise_nb or ""}'
           f'-w.{want or "none"}{"-nopart" if nopart else ""}-acc{acc}{"-g4B" if og else ""}{"-ref4B" if oref else ""}'
           f'{"-gx4B" if ogx else ""}{note}')
    return case(id='bab-' + tag, N=N, hw=hw, C=C, rows=rows, noise_nb=noise_nb, want=want, acc=acc, og=og, oref=oref, ogx=ogx,
                nopart=nopart, vec=vec, plan=pl)


# 300 is a multiple of 4: it takes the vector form with cg = 75, rpb = 3 (31 idle threads); 302 is the scalar two-chunk shape
VEC_C, SCALAR_C = (4, 12, 40, 64, 300, 512, 1024, 1028, 2048), (1, 3, 257, 302)
BIG_ROWS_C = (4, 12, 40, 64, 1, 3)         # rows = 8192 / 8200 (exact fill of 512 blocks / 29 empty blocks) stay below ~2 MB


def _bab_cases():
    out = []
    # vector / scalar x column chunks x block layouts: one block, exact fill, short last block; 512 blocks; empty blocks
    for C in VEC_C + SCALAR_C:
        for rows in (1, 15, 16, 17, 100, 197):               # 197: 13 blocks of 16 rows, the last of 5
            if C == 1 and rows == 1:
                continue                       # a single element: nothing to tell apart
            out.append(_bab(1, rows, C, want='b'))
        if C in BIG_ROWS_C:
            out += [_bab(1, 8192, C, want='b'), _bab(1, 8200, C, want='b'), _bab(8, 1025, C, noise_nb=2, want='bw')]
    # the scalar form at an aligned C % 4 == 0, forced by one pointer 4 bytes off
    for off in ({'og': 1}, {'oref': 1}, {'ogx': 1}):
        out += [_bab(1, 100, 64, want='b', **off), _bab(4, 25, 64, noise_nb=2, want='bw', **off)]
    # noise index: per sample / shared (1 map, 3 images) / wrapped (2 maps, 4 images) at 5 x 5 images, whose boundaries fall
    # inside a block: C >= 512 walks them in the unrolled loop (rpb <= 2), C = 302's first chunk in the remainder loop (rpb = 1)
    for C in (64, 512, 1028, 2048, 300, 302, 3):
        out += [_bab(3, 25, C, noise_nb=3, want='bw'), _bab(3, 25, C, noise_nb=1, want='bw'), _bab(4, 25, C, noise_nb=2, want='bw'),
                _bab(1, 25, C, noise_nb=1, want='w')]
    # rpb > rows_per_img: the wrap loop runs several times per step.  C = 4 with 4 x 4 images (one row per thread: the start
    # index); C = 1 with 200 000 rows (rows per block 391 > rpb = 256: a second remainder trip uses the wrapped index); C = 4
    # with 400 000 rows (rows per block 782 > 3 * 256: the unrolled loop uses it) — the only shapes that reach those trips
    out += [_bab(40, 16, 4, noise_nb=1, want='bw'), _bab(40, 16, 4, noise_nb=2, want='bw'), _bab(40, 16, 4, noise_nb=40, want='bw'),
            _bab(8000, 25, 1, noise_nb=3, want='bw', note='-multiwrap'), _bab(16000, 25, 4, noise_nb=3, want='bw', note='-multiwrap')]
    # wanted set x accumulate
    for N, hw, C in ((4, 25, 64), (4, 25, 1028), (4, 25, 302), (8, 1025, 12)):
        for want in ('b', 'w', 'bw', ''):
            for acc in (0, 1, 2):
                if want or acc == 0:
                    out.append(_bab(N, hw, C, noise_nb=2, want=want, acc=acc))
        out.append(_bab(N, hw, C, noise_nb=0, want='', nopart=True))
        out.append(_bab(N, hw, C, noise_nb=2, want='', nopart=True))
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


def _dot(N, hw, C, noise_nb, bias, nw, want='bw'):
    rows = N * hw
    pl = bab_plan(rows, C, True)
    assert dot_ok(rows, C, hw)
    bpi = pl.nb // N
    tag = (f'C{C}-N{N}x{hw}-nb{pl.nb}x{pl.rpblk}-ch{"+".join(f"{cg}x{rpb}" for cg, rpb in pl.chunks)}-bpi{bpi}-t{_trips(dot_reduce_trips(bpi))}'
           f'-nz.{noise_path(N, noise_nb)}{noise_nb or ""}{"-bias" if bias else ""}{"-nw" if nw else ""}-w.{want or "none"}')
    return case(id='dot-' + tag, N=N, hw=hw, C=C, rows=rows, noise_nb=noise_nb, bias=bias, nw=nw, want=want, acc=0, og=0, oref=0, ogx=0,
                nopart=False, vec=True, plan=pl, bpi=bpi)


def _dot_cases():
    out = []
    for N, hw, C in ((3, 16, 64), (2, 32, 1028)):                     # bpi = 1 / 2; 1028: the chunked DOT store (dbias at cbase)
        for bias in (True, False):
            for nw in (True, False):
                out.append(_dot(N, hw, C, N if nw or bias else 1, bias, nw))
        out += [_dot(N, hw, C, 0, True, False, want='b'), _dot(N, hw, C, 1, True, True, want='')]
    # bpi = 16, 40, 96, 512 (the two-way loop of bab_dot_reduce_kernel changes shape at 32 and 64); 512 blocks of 32 rows
    for N, hw, C in ((2, 256, 8), (2, 640, 8), (2, 1536, 8), (1, 8192, 8), (1, 16384, 4), (3, 16, 40), (2, 32, 512), (2, 32, 2048)):
        out += [_dot(N, hw, C, N, True, True), _dot(N, hw, C, 1, False, True, want='w')]
    return out


def _spl(N, hw, C, form, noise_nb=0, want='b'):
    rows = N * hw
    pl = bab_plan(rows, C, True)
    tag = f'C{C}-N{N}x{hw}-nb{pl.nb}x{pl.rpblk}-ch{"+".join(f"{cg}x{rpb}" for cg, rpb in pl.chunks)}-{form}-nz.{noise_path(N, noise_nb)}-w.{want or "none"}'
    return case(id='spl-' + tag, N=N, hw=hw, C=C, rows=rows, noise_nb=noise_nb, want=want, form=form, acc=0, og=0, oref=0, ogx=0,
                nopart=False, vec=True, plan=pl)


SPL_FORMS = ('out1', 'out1+out2', 'cs', 'cs+f32', 'out1+out2+f32')


def _spl_cases():
    # C = 36: not a multiple of 32 — the entry takes any C % 4 == 0 and writes rick_split_pack_f32's image (the contract this pins)
    wants = ('b', 'bw', '', 'w', 'bw')
    return [_spl(2, 25, C, form, noise_nb=2 if 'w' in wants[i] else 0, want=wants[i])
            for C in (32, 128, 1056, 36) for i, form in enumerate(SPL_FORMS)] + [_spl(1, 100, 128, 'out1+out2'), _spl(1, 17, 32, 'cs+f32')]


BAB, DOT, SPL = _bab_cases(), _dot_cases(), _spl_cases()


# ------------------------------------------------------------------------------------------------- backward: builders
def build_bab(c, mode):
    """gx: one product and two roundings (the slope, the scale): n = 1, k = 1.  gb: rows terms, each o rounded twice: k = 2.
    gnw: rows * C terms o * noise — o's two roundings and the product (the lane's four-channel sum is part of the summation):
    k = 3.  The per-block partial rows: the same with the block's rows.
    gd (DOT): hw terms o * t per (image, channel), t = unact(y) - nw * noise - bias expanded into its three products: o's two
    roundings, the rounded scale * alpha, its reciprocal, the un-activation product, the nw * noise product and the two
    subtractions: k = 8 (hw_dot_act's 5 + o's 2 + the noise product), + 1 for the division."""
    rows, C, N, hw = c.rows, c.C, c.N, c.hw
    g = fill(c.id + '/g', (rows, C), mode, 3)
    ref = fill(c.id + '/ref', (rows, C), mode, 6)
    if rows * C >= 2:                       # mixed signs and distinct outputs whatever the draw
        gf, rf = g.view(-1), ref.view(-1)
        gf[0], gf[1] = (1.0, 2.0) if mode == 'exact' else (float(gf[0].abs()) + 0.5, -float(gf[1].abs()) - 1.5)
        rf[0], rf[1] = float(rf[0].abs()) + 1.0, -float(rf[1].abs()) - 1.0
        assert float(ref.min()) < 0 < float(ref.max()), 'ref must have mixed signs'
    alpha, scale = (0.25, 2.0) if mode == 'exact' else (f32(0.2), f32(math.sqrt(2)))
    o = g.double() * torch.where(ref > 0, 1.0, alpha).double() * scale
    unit = alpha * scale
    b = types.SimpleNamespace(g=g, ref=ref, alpha=alpha, scale=scale, o=o, noise=None, nz=None, unit=unit)
    self_check(mode, o if rows * C > 1 else o.new_tensor([0.0, 1.0]), o.abs(), unit)
    b.gb, b.Sgb = o.sum(0), o.abs().sum(0)
    self_check(mode, b.gb if C > 1 else o, b.Sgb, unit)
    if c.noise_nb:
        b.noise = fill(c.id + '/noise', (c.noise_nb, hw), mode, 2)
        r = torch.arange(rows)
        b.nz = b.noise.double()[(r // hw) % c.noise_nb, r % hw]          # [rows]
        b.onz = o * b.nz[:, None]
        b.gnw, b.Sgnw = b.onz.sum().reshape(1), b.onz.abs().sum().reshape(1)
        self_check(mode, b.onz, b.Sgnw, unit)
    return b


def build_dot(c, mode):
    b = build_bab(c, mode)
    N, hw, C = c.N, c.hw, c.C
    y = b.ref.double()
    t = torch.where(y > 0, y / b.scale, y / (b.scale * b.alpha))
    T = t.abs()
    b.bias = b.nw = None
    if c.bias:
        b.bias = fill(c.id + '/bias', (C,), mode, 3, nonzero=True)
        t, T = t - b.bias.double(), T + b.bias.double().abs()
    if c.nw:
        b.nw = torch.tensor([-2.0]) if mode == 'exact' else synth_tensor('forms/' + c.id + '/nw', (1,))
        nv = float(b.nw) * b.nz[:, None]
        t, T = t - nv, T + nv.abs()
    b.div = divisor_for(c, mode)
    gd, Sgd = (b.o * t).view(N, hw, C).sum(1), (b.o.abs() * T).view(N, hw, C).sum(1)
    self_check(mode, gd, Sgd, b.unit * 0.5)           # o in units of alpha * scale, t in halves
    b.gd, b.Sgd = gd / b.div.double(), Sgd / b.div.double().abs()
    return b


# ------------------------------------------------------------------------------------------------ column sums: tables
def _cs(rows, ncols, pad, acc):
    cpb, G, trips = colsum_plan(rows, ncols)
    return case(id=f'colsum-cpb{cpb}g{G}-rows{rows}-ncols{ncols}-stride{ncols + pad}-t{_trips(trips)}{"-acc" if acc else ""}', rows=rows,
                ncols=ncols, stride=ncols + pad, acc=acc, cpb=cpb, trips=trips)


def _colsum_cases():
    out, i = [], 0
    for ncols, rowset in ((2, (1, 31, 32, 33, 96, 97, 128, 129, 700)), (7, (1, 31, 32, 33, 96, 97, 128, 129, 700)),
                          (8, (1, 31, 32, 33, 96, 97, 128, 129, 700)), (9, (1, 31, 32, 33, 96, 97, 128, 129, 700)),
                          (513, (1, 33, 97, 129, 700)), (1, (1, 255, 256, 257, 768, 769, 1024, 1500, 1800))):
        for rows in rowset:
            out += [_cs(rows, ncols, 3 * (i % 2), bool(i // 2 % 2)), _cs(rows, ncols, 3 * ((i + 1) % 2), not i // 2 % 2)]
            i += 1
    return out


# (nb, ncols, pad, col0, split (0: no out2), accumulate) — single- and multi-column items, col0 > 0, out2 / split, accumulate
MULTI_TEMPLATES = [(33, 9, 0, 0, 0, 0), (257, 1, 4, 3, 0, 0), (129, 17, 3, 2, 16, 0), (1, 8, 0, 0, 0, 1), (700, 1, 0, 0, 0, 1),
                   (97, 7, 2, 1, 0, 1), (16, 65, 0, 0, 64, 1), (1025, 1, 1, 1, 0, 0), (128, 24, 0, 0, 0, 0), (5, 2, 1, 1, 1, 0)]
MULTI = [case(id=f'multi-{n}items-{-(-n // COLSUM_MAX)}launches', n=n) for n in (1, 32, 33, 70)]


def multi_items(n):
    return [MULTI_TEMPLATES[(i * 3 + i // len(MULTI_TEMPLATES)) % len(MULTI_TEMPLATES)] for i in range(n)]


COLSUM = _colsum_cases()


def build_colsum(key, mode, rows, stride, ncols, col0, acc):
    part = fill(key + '/part', (rows, stride), mode, 50)
    old = fill(key + '/old', (ncols,), mode, 50, nonzero=True) if acc else None
    cols = part.double()[:, col0:col0 + ncols]
    ref, S = cols.sum(0), cols.abs().sum(0)
    if acc:
        ref, S = ref + old.double(), S + old.double().abs()
    self_check(mode, ref if ncols > 1 else cols if rows > 1 else ref.new_tensor([0.0, 1.0]), S)
    return types.SimpleNamespace(part=part, old=old, ref=ref, S=S, n=rows + int(acc), k=0)


# --------------------------------------------------------------------------------------------------- forward: tables
FWD_MODES = {'lrelu': (3, 0), 'lrelu_grad': (3, 1), 'lrelu_grad2': (3, 2), 'linear_grad2': (1, 2), 'linear': (1, 0)}


def _fwd(N, HW, C, mode='lrelu', bias=True, noise_nb=0, planar=False, ox=0, oout=0, oref=0, note=''):
    n = N * HW * C
    step_b, n_div, hw_div = (HW, C * HW, 1) if planar else (1, HW * C, C)
    vec, blocks, second = fwd_plan(n, bias, step_b, C, bool(noise_nb), n_div, hw_div, aligned=not (ox or oout or oref))
    tag = (f'{"vec" if vec else "scalar"}-{mode}-N{N}-HW{HW}-C{C}{"-planar" if planar else ""}{"-bias" if bias else ""}'
           f'{f"-noise{noise_nb}" if noise_nb else ""}{"-x4B" if ox else ""}{"-out4B" if oout else ""}{"-ref4B" if oref else ""}'
           f'-blocks{blocks}{"-gridstride" if second else ""}{note}')
    return case(id='fwd-' + tag, N=N, HW=HW, C=C, n=n, mode=mode, bias=bias, noise_nb=noise_nb, planar=planar, ox=ox, oout=oout, oref=oref,
                step_b=step_b, n_div=n_div, hw_div=hw_div, vec=vec, blocks=blocks, second=second, why=note)


def _fwd_cases():
    out = []
    for mode in FWD_MODES:
        for bias, nnb in ((True, 2), (True, 0), (False, 3), (False, 0)):
            out += [_fwd(3, 25, 8, mode, bias, nnb), _fwd(3, 25, 3, mode, bias, nnb, note='-n%4')]
    for mode in ('lrelu', 'lrelu_grad'):
        out += [_fwd(2, 16, 4, mode, True, 0, planar=True, note='-step_b'), _fwd(2, 16, 4, mode, True, 2, planar=True, note='-step_b'),
                _fwd(2, 10, 6, mode, False, 2, note='-hw_div%4'), _fwd(3, 25, 8, mode, True, 3, ox=1, note='-ptr'),
                _fwd(3, 25, 8, mode, True, 3, oout=1, note='-ptr'), _fwd(3, 25, 8, mode, False, 0, ox=1, note='-ptr')]
    out.append(_fwd(3, 25, 8, 'lrelu_grad', True, 3, oref=1, note='-ptr'))
    out += [_fwd(1, 300, 1028, 'lrelu', True, 1), _fwd(2, 1025, 12, 'lrelu_grad', True, 2)]
    # past the grid cap of 4096 blocks: 4 194 304 floats (vector) / 1 048 576 floats (scalar) fill one sweep
    out += [_fwd(1, 65541, 64, 'lrelu', True, 1, note='-gridcap'), _fwd(1, 349531, 3, 'lrelu', True, 1, note='-gridcap')]
    return out


FWD = _fwd_cases()


def build_fwd(c, mode):
    """y = act(x + bias + nw * noise) * scale: up to three summed terms (n), the nw * noise product, the slope and the scale
    (k = 3).  lrelu selects by the sign of the fp32 sum: where that differs from the fp64 sign, |v| is below its own rounding
    error and both branches lie inside the bound."""
    N, HW, C, n = c.N, c.HW, c.C, c.n
    act, grad = FWD_MODES[c.mode]
    x = fill(c.id + '/x', (n,), mode, 20)
    i = torch.arange(n)
    ch, pixel, img = ((i // HW) % C, i % HW, i // (C * HW)) if c.planar else (i % C, (i // C) % HW, i // (HW * C))
    alpha, scale = (0.25, 2.0) if mode == 'exact' else (f32(0.2), f32(math.sqrt(2)))
    b = types.SimpleNamespace(x=x, bias=None, noise=None, nw=None, ref_in=None, alpha=alpha, scale=scale, act=act, grad=grad, n=1, k=3)
    v, S = x.double(), x.double().abs()
    if c.bias:
        b.bias = fill(c.id + '/bias', (C,), mode, 9, nonzero=True)
        v, S, b.n = v + b.bias.double()[ch], S + b.bias.double().abs()[ch], b.n + 1
    if c.noise_nb:
        b.noise = fill(c.id + '/noise', (c.noise_nb, HW), mode, 2)
        b.nw = torch.tensor([-2.0]) if mode == 'exact' else synth_tensor('forms/' + c.id + '/nw', (1,))
        nv = float(b.nw) * b.noise.double()[img % c.noise_nb, pixel]
        v, S, b.n = v + nv, S + nv.abs(), b.n + 1
    if (act, grad) == (3, 1):
        b.ref_in = fill(c.id + '/ref', (n,), mode, 6)
        b.ref_in[0], b.ref_in[1] = 1.0, -1.0
        sel = b.ref_in > 0
    else:
        sel = v > 0
    if grad == 2:
        y, S = torch.zeros_like(v), torch.zeros_like(v)
    elif act == 3:
        y, S = torch.where(sel, v, v * alpha) * scale, S * scale
    else:
        y, S = v * scale, S * scale
    if grad != 2:
        self_check(mode, y, S, alpha * scale)
        assert float(y.min()) < 0 < float(y.max())
    b.ref, b.S = y, S
    return b


# ---------------------------------------------------------------------------------------------------- host-only tests
def _load_lib():
    try:
        from rick_amd._lib import lib
        return lib
    except OSError:
        return None


def test_replay_agrees_with_the_library_and_every_listed_branch_has_a_case():
    lib = _load_lib()
    assert len({c.id for c in BAB + DOT + SPL + COLSUM + FWD}) == len(BAB + DOT + SPL + COLSUM + FWD)
    for c in BAB + DOT + SPL:
        assert c.vec == (c.C % 4 == 0 and not (c.og or c.oref or c.ogx)), c.id
        pl = bab_plan(c.rows, c.C, c.vec)
        assert (pl.nb, pl.rpblk) == (max(1, min(-(-c.rows // 16), 512)), -(-c.rows // pl.nb)) and f'-nb{pl.nb}x{pl.rpblk}-' in c.id, c.id
        assert ('vec' in c.id) == c.vec or not c.id.startswith('bab-'), c.id
        if lib is not None:
            assert lib.rick_bias_act_bwd_blocks(c.rows, c.C) == pl.nb, c.id
            assert lib.rick_bias_act_bwd_dot_ok(c.rows, c.C, c.hw) == dot_ok(c.rows, c.C, c.hw), c.id
    if lib is not None:
        for rows, C, hw in ((75, 64, 25), (48, 6, 16), (8200, 8, 1025), (16384, 4, 16384), (1280, 8, 640), (100, 8, 30)):
            assert lib.rick_bias_act_bwd_dot_ok(rows, C, hw) == dot_ok(rows, C, hw), (rows, C, hw)
    # vector / scalar and column chunks
    vec_c = {c.C for c in BAB if c.vec}
    assert vec_c >= set(VEC_C) and {c.C for c in BAB if not c.vec and c.C % 4} >= set(SCALAR_C)
    assert {(bool(c.og), bool(c.oref), bool(c.ogx)) for c in BAB if not c.vec and c.C == 64} == {(True, False, False), (False, True, False),
                                                                                                   (False, False, True)}
    chunks = {tuple(c.plan.chunks) for c in BAB}
    assert {((1, 256),), ((3, 85),), ((10, 25),), ((16, 16),), ((128, 2),), ((256, 1),), ((256, 1), (1, 256)), ((256, 1), (256, 1)),
            ((75, 3),), ((256, 1), (46, 5))} <= chunks
    assert ((256, 1), (8, 32)) in {tuple(c.plan.chunks) for c in SPL} and ((256, 1), (1, 256)) in {tuple(c.plan.chunks) for c in DOT}
    # rows: one block / exact fill / short last block / 512 blocks / empty blocks; unrolled only, remainder only, both
    layouts = {(c.plan.nb, c.plan.rpblk, c.plan.nonempty) for c in BAB}
    assert {(1, 1, 1), (1, 15, 1), (1, 16, 1), (2, 9, 2), (7, 15, 7), (512, 16, 512), (512, 17, 483)} <= layouts
    assert any('empty' in c.plan.trips and c.noise_nb for c in BAB) and any('empty' in c.plan.trips and not c.noise_nb for c in BAB)
    for vec in (True, False):
        trips = set().union(*(s for c in BAB if c.vec == vec for k, s in c.plan.trips.items() if k != 'empty'))
        assert any(u == 0 and m > 1 for u, m in trips) and (0, 0) in trips
        if vec:
            assert any(u > 0 and m == 0 for u, m in trips) and any(u > 1 and m > 0 for u, m in trips), trips
            assert any(len({u for u, _ in c.plan.trips['first']}) > 1 for c in BAB if c.vec)      # trip counts differ per thread row
        else:
            assert all(u == 0 for u, _ in trips)
    assert all(s == {(0, 0)} for c in BAB if 'empty' in c.plan.trips for s in [c.plan.trips['empty']])
    # noise paths, the wrap loop inside both loops, its reset, and several iterations per step
    assert {(noise_path(c.N, c.noise_nb), c.vec) for c in BAB} >= {(pth, v) for pth in ('none', 'persample', 'shared', 'wrapped') for v in (True, False)}
    assert any(c.noise_nb == 1 and c.N == 3 for c in BAB) and any(c.noise_nb == 2 and c.N == 4 for c in BAB)
    assert any(c.C == 4 and c.hw == 16 and c.N == 40 for c in BAB)
    walked = {}
    for c in BAB:
        if noise_path(c.N, c.noise_nb) in ('shared', 'wrapped'):
            walked[c.id] = noise_walk(c.rows, c.C, c.vec, c.hw, c.noise_nb)
    allw = set().union(*walked.values())
    assert {('U', 1, True), ('R', 1, True), ('U', 1, False), ('R', 1, False), ('U', 0, False), ('R', 0, False)} <= allw, allw
    assert {('U', 2, True), ('R', 2, True)} <= allw, 'no case uses an index that the wrap loop advanced more than once'
    assert all(any(it == 2 for _, it, _ in walked[c.id]) and min(r for _, r in c.plan.chunks) > c.hw for c in BAB if 'multiwrap' in c.id)
    # wanted set x accumulate
    assert {(c.want, c.acc) for c in BAB} >= {(w, a) for w in ('b', 'w', 'bw') for a in (0, 1, 2)} | {('', 0)}
    assert any(c.nopart and c.noise_nb for c in BAB) and any(c.nopart and not c.noise_nb for c in BAB)
    # DOT
    assert {c.bpi for c in DOT} >= {1, 16, 40, 96, 512} and any(c.C == 1028 for c in DOT)
    assert {(c.bias, c.nw) for c in DOT} == {(a, b) for a in (True, False) for b in (True, False)}
    assert {(c.bias, c.nw) for c in DOT if c.C == 1028} == {(a, b) for a in (True, False) for b in (True, False)}
    dt = {c.bpi: dot_reduce_trips(c.bpi) for c in DOT}
    assert dt[16] == {(0, 1), (0, 0)} and dt[40] == {(1, 0), (0, 1)} and dt[96] == {(1, 1)} and dt[512] == {(8, 0)}
    assert any(c.plan.rpblk > 16 for c in DOT)
    # SPL
    assert {(c.C, c.form) for c in SPL} >= {(C, f) for C in (32, 128, 1056, 36) for f in SPL_FORMS}
    # column sums
    assert {(c.ncols, c.rows) for c in COLSUM} >= {(nc, r) for nc in (2, 7, 8, 9) for r in (1, 31, 32, 33, 96, 97, 128, 129, 700)} | \
        {(1, r) for r in (1, 255, 256, 257, 768, 769, 1024, 1500)} | {(513, 700)}
    for ncols in (1, 8, 513):
        assert {(c.stride > c.ncols, c.acc) for c in COLSUM if c.ncols == ncols} == {(a, b) for a in (True, False) for b in (True, False)}
    for cpb in (1, 8):
        trips = set().union(*(c.trips for c in COLSUM if c.cpb == cpb))
        assert {(0, 0), (0, 1), (0, 3), (1, 0), (1, 1)} <= trips and any(u > 0 and m > 1 for u, m in trips), (cpb, trips)
    assert [c.n for c in MULTI] == [1, 32, 33, 70]
    its = multi_items(70)
    assert {t[1] == 1 for t in its} == {True, False} and any(t[3] for t in its) and any(t[4] for t in its) and any(t[5] for t in its)
    for batch in (its[:32], its[32:64], its[64:]):                  # both kernel forms in every launch of the 70
        assert {t[1] == 1 for t in batch} == {True, False}
    # forward
    assert {(c.vec, c.mode, c.bias, bool(c.noise_nb)) for c in FWD} >= {(v, m, b, z) for v in (True, False) for m in FWD_MODES
                                                                       for b in (True, False) for z in (True, False)}
    assert {c.why for c in FWD if not c.vec} >= {'-n%4', '-step_b', '-hw_div%4', '-ptr', '-gridcap'}
    assert {c.vec for c in FWD if c.second} == {True, False} and all(c.blocks == EW_GRID_CAP for c in FWD if c.second)
    for c in FWD:
        if c.why == '-hw_div%4':
            assert c.n % 4 == 0 and not c.bias and c.hw_div % 4
        if c.why == '-step_b':
            assert c.n % 4 == 0 and c.C % 4 == 0 and c.step_b != 1
        if c.why == '-ptr':
            assert fwd_plan(c.n, c.bias, c.step_b, c.C, bool(c.noise_nb), c.n_div, c.hw_div)[0]


@pytest.mark.parametrize('family', ['bab', 'dot', 'spl', 'colsum', 'multi', 'fwd'])
def test_case_tables_are_exact_and_not_degenerate(family):
    """No device: the exact-mode inputs of every case satisfy sum |terms| < 2**24 units, `ref` has mixed signs and the expected
    outputs are not constant (asserted inside the builders).  The two grid-cap and the two 10**5-row cases: on the device only."""
    if family == 'colsum':
        for c in COLSUM:
            build_colsum(c.id, 'exact', c.rows, c.stride, c.ncols, 0, c.acc)
    elif family == 'multi':
        for i, (nb, ncols, pad, col0, split, acc) in enumerate(multi_items(70)):
            build_colsum(f'multi/{i}', 'exact', nb, ncols + pad + col0, ncols, col0, acc)
    elif family == 'fwd':
        for c in FWD:
            if c.n <= 1 << 20:
                build_fwd(c, 'exact')
    else:
        for c in {'bab': BAB, 'dot': DOT, 'spl': SPL}[family]:
            if c.rows * c.C <= 1 << 20:
                (build_dot if family == 'dot' else build_bab)(c, 'exact')


# ----------------------------------------------------------------------------------------------------- device helpers
def out_buf(numel, old=None, off=0):
    return Guarded(numel, off, old)


def all_sentinel(*bufs):
    return all(bool((g.buf == SENT).all()) for g in bufs if g is not None)


def check_partials(c, mode, part, b, want_b, want_w):
    """The per-block rows [blocks][C + 1]: bias columns written only when gb is wanted, column C only when gnw is; the rows of
    empty blocks are zeros; everything else keeps the sentinel."""
    pl, C = c.plan, c.C
    P = part.v.detach().cpu().view(pl.nb, C + 1)
    blk = torch.arange(c.rows) // pl.rpblk
    if want_b:
        ref = torch.zeros(pl.nb, C, dtype=torch.float64).index_add_(0, blk, b.o)
        S = torch.zeros(pl.nb, C, dtype=torch.float64).index_add_(0, blk, b.o.abs())
        compare(c, mode, P[:, :C], ref, S, pl.rpblk, 2, 'partials[:, :C]')
        assert bool((P[pl.nonempty:, :C] == 0).all()), 'an empty block did not write zero partials'
    else:
        assert bool((P[:, :C] == SENT).all()), 'bias partials written though gb was not wanted'
    if want_w:
        ref = torch.zeros(pl.nb, dtype=torch.float64).index_add_(0, blk, b.onz.sum(1))
        S = torch.zeros(pl.nb, dtype=torch.float64).index_add_(0, blk, b.onz.abs().sum(1))
        compare(c, mode, P[:, C], ref, S, pl.rpblk * C, 3, 'partials[:, C]')
        assert bool((P[pl.nonempty:, C] == 0).all())
    else:
        assert bool((P[:, C] == SENT).all()), 'noise partial written though gnw was not wanted'


def launch_bab(c, b, acc, old_b=None, old_w=None, dot=None):
    """One launch of rick_bias_act_bwd_f32 (or _dot_f32) on fresh guarded buffers -> namespace of the buffers and rc."""
    from rick_amd._lib import lib
    C, rows = c.C, c.rows
    r = types.SimpleNamespace()
    r.g, r.ref, r.noise = dev_in(b.g, c.og), dev_in(b.ref, c.oref), dev_in(b.noise)
    r.gx = out_buf(rows * C, off=c.ogx)
    r.part = None if c.nopart else out_buf(c.plan.nb * (C + 1))
    r.gb = out_buf(C, old_b) if 'b' in c.want else None
    r.gnw = out_buf(1, old_w) if 'w' in c.want else None
    args = (p(r.g), p(r.ref), p(r.gx), p(r.gb), p(r.gnw), p(r.noise), rows, C, c.hw, max(c.noise_nb, 1), c.hw, b.alpha, b.scale, p(r.part), acc)
    if dot is None:
        r.rc = lib.rick_bias_act_bwd_f32(*args, stream())
    else:
        r.bias, r.nw, r.div = dev_in(b.bias), dev_in(b.nw), dev_in(b.div)
        r.gd, r.dpart = out_buf(c.N * C), out_buf(c.plan.nb * C)
        r.rc = lib.rick_bias_act_bwd_dot_f32(*args, p(r.bias), p(r.nw), p(r.div), p(r.gd), p(r.dpart), stream())
    torch.cuda.synchronize()
    return r


def check_bab(c, mode, b, r, old_b=None, old_w=None, written=True, nz_read=False):
    r.gx.assert_bands(c.id + ' gx')
    compare(c, mode, r.gx.v, b.o, b.o.abs(), 1, 1, 'gx')
    if r.part is not None:
        r.part.assert_bands(c.id + ' partials')
        check_partials(c, mode, r.part, b, 'b' in c.want, 'w' in c.want or nz_read)
    for name, buf, ref, S, old, n, k in (('gb', r.gb, b.gb, b.Sgb, old_b, c.rows, 2),
                                          ('gnw', r.gnw, getattr(b, 'gnw', None), getattr(b, 'Sgnw', None), old_w, c.rows * c.C, 3)):
        if buf is None:
            continue
        buf.assert_bands(c.id + ' ' + name)
        if not written:
            assert bool((buf.v == SENT).all()), f'{name} written under accumulate = 2'
            continue
        if old is not None:
            ref, S, n = ref + old.double(), S + old.double().abs(), n + 1
        compare(c, mode, buf.v, ref, S, n, k, name)


# -------------------------------------------------------------------------------------------------- GPU: the backward
@gpu
@pytest.mark.parametrize('mode', MODES)
@params(BAB)
def test_bias_act_bwd_forms(c, mode):
    from rick_amd._lib import ColsumItem, lib
    assert lib.rick_bias_act_bwd_blocks(c.rows, c.C) == c.plan.nb
    b = build_bab(c, mode)
    old_b = fill(c.id + '/oldb', (c.C,), mode, 50, nonzero=True) if c.acc == 1 else None
    old_w = fill(c.id + '/oldw', (1,), mode, 50, nonzero=True) if c.acc == 1 else None
    r = launch_bab(c, b, c.acc, old_b, old_w)
    assert r.rc == 0
    check_bab(c, mode, b, r, old_b, old_w, written=c.acc != 2)
    if c.acc != 2:
        return
    # accumulate = 2: the destinations are untouched; rick_colsum_multi_f32 over the partial rows gives the immediate result
    item = ColsumItem(p(r.part), p(r.gb) if r.gb else p(r.gnw), p(r.gnw) if r.gb and r.gnw else None, c.plan.nb, c.C + 1,
                      (c.C if r.gb else 0) + (1 if r.gnw else 0), 0 if r.gb else c.C, c.C if r.gb and r.gnw else 0, 0)
    assert lib.rick_colsum_multi_f32(ctypes.byref(item), 1, stream()) == 0
    torch.cuda.synchronize()
    check_bab(c, mode, b, r)
    now = launch_bab(c, b, 0)
    assert now.rc == 0
    for deferred, immediate in ((r.gb, now.gb), (r.gnw, now.gnw)):
        assert deferred is None or torch.equal(deferred.v, immediate.v), 'deferred column sum != the immediate one'


@gpu
def test_bias_act_bwd_rejects_what_it_has_no_path_for():
    """gnw without noise, noise_hw != rows_per_img, gb without partials: RICK_EINVAL, every buffer still at the sentinel."""
    from rick_amd._lib import lib
    rows, C, hw = 50, 8, 25
    g, ref, noise = Guarded(rows * C), Guarded(rows * C), Guarded(2 * hw)
    gx, gb, gnw, part = Guarded(rows * C), Guarded(C), Guarded(1), Guarded(bab_blocks(rows) * (C + 1))

    def call(gb_, gnw_, noise_, noise_hw, part_):
        return lib.rick_bias_act_bwd_f32(p(g), p(ref), p(gx), p(gb_), p(gnw_), p(noise_), rows, C, hw, 2, noise_hw, 0.25, 2.0, p(part_), 0,
                                         stream())
    assert call(gb, gnw, None, hw, part) == EINVAL
    assert call(gb, gnw, noise, hw + 1, part) == EINVAL
    assert call(gb, None, None, hw, None) == EINVAL
    torch.cuda.synchronize()
    assert all_sentinel(gx, gb, gnw, part)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(DOT)
def test_bias_act_bwd_dot_forms(c, mode):
    from rick_amd._lib import lib
    assert lib.rick_bias_act_bwd_dot_ok(c.rows, c.C, c.hw) == 1
    b = build_dot(c, mode)
    r = launch_bab(c, b, 0, dot=True)
    assert r.rc == 0
    check_bab(c, mode, b, r, nz_read=c.nw)         # (the noise partial is written whenever the pass reads the noise values)
    r.gd.assert_bands(c.id + ' gd')
    r.dpart.assert_bands(c.id + ' dpartials')
    assert not bool((r.dpart.v == SENT).any()), 'a dpartials row was never written'
    compare(c, mode, r.gd.v, b.gd, b.Sgd, c.hw, (8 if mode == 'bound' else 0) + 1, 'gd')
    plain = launch_bab(c, b, 0)
    assert plain.rc == 0
    for a, bb in ((r.gx, plain.gx), (r.gb, plain.gb), (r.gnw, plain.gnw)):
        assert a is None or torch.equal(a.v, bb.v), 'the DOT form changed gx / gb / gnw'


@gpu
def test_bias_act_bwd_dot_rejections():
    """A block would straddle an image (dot_ok == 0), an offset pointer, alpha == 0, noise_w without noise."""
    from rick_amd._lib import lib
    C = 8
    bufs = []

    def call(N, hw, og=0, alpha=0.25, noise=False, nw=False):
        rows = N * hw
        g, ref, gx = Guarded(rows * C, og), Guarded(rows * C), Guarded(rows * C)
        nb = bab_blocks(rows)
        part, dpart, gd, div, w, nz = Guarded(nb * (C + 1)), Guarded(nb * C), Guarded(N * C), Guarded(N * C), Guarded(1), Guarded(hw)
        bufs.extend([gx, part, dpart, gd])
        return lib.rick_bias_act_bwd_dot_f32(p(g), p(ref), p(gx), None, None, p(nz) if noise else None, rows, C, hw, 1, hw, alpha, 2.0, p(part), 0,
                                             None, p(w) if nw else None, p(div), p(gd), p(dpart), stream())
    assert dot_ok(75, C, 25) == 0 and lib.rick_bias_act_bwd_dot_ok(75, C, 25) == 0 and call(3, 25) == EINVAL
    assert dot_ok(48, C, 16) == 1
    assert call(3, 16, og=1) == EINVAL
    assert call(3, 16, alpha=0.0) == EINVAL
    assert call(3, 16, nw=True) == EINVAL
    torch.cuda.synchronize()
    assert all_sentinel(*bufs)


# ------------------------------------------------------------------------------------------ GPU: the split-image form
def amax_word(value):
    """A running-maximum word whose value sits in a slot other than the first (readers take the maximum over the slots)."""
    w = torch.zeros(AMAX_FLOATS)
    w[0], w[5 * AMAX_STRIDE] = value / 2, value
    return Guarded(AMAX_FLOATS, 0, w)


def pack_reference(x32, word, coef, rows, C):
    from rick_amd._lib import lib
    src, img, hdr = dev_in(x32), Guarded(rows * C), Guarded(4)
    assert lib.rick_split_pack_f32(p(src), p(img), p(hdr), p(word), None, coef, rows, C, stream()) == 0
    return img, hdr


def check_image(c, mode, img, hdr, x32, x64, word, coef, what):
    """The image and the first three header words == rick_split_pack_f32 of the reference under the same bound word and
    coefficient, bit for bit; unpacked, it stays within the format's step of the fp64 reference."""
    from rick_amd._lib import lib
    rows, C = c.rows, c.C
    img.assert_bands(f'{c.id} {what}')
    hdr.assert_bands(f'{c.id} {what} header')
    rimg, rhdr = pack_reference(x32, word, coef, rows, C)
    torch.cuda.synchronize()
    assert torch.equal(hdr.v[:3], rhdr.v[:3]), f'{what}: header {hdr.v.tolist()} != {rhdr.v.tolist()}'
    assert torch.equal(img.v.view(torch.int32), rimg.v.view(torch.int32)), f'{what}: image differs from the standalone pack'
    back = Guarded(rows * C)
    assert lib.rick_split_unpack_f32(p(img), p(hdr), p(back), rows, C, stream()) == 0
    torch.cuda.synchronize()
    bound = float(hdr.v[2])
    # |x - hi - lo| <= 2^-22 |x| within 2^10 of the bound, 2^-25 / 2^13 of the bound below (tests/test_gpu_split.py); + the three
    # roundings of the value itself (slope, scale, chan_scale) in bound mode
    tol = torch.maximum(x64.abs() * (2.0 ** -21 + (3 * U if mode == 'bound' else 0.0)), torch.full_like(x64, bound * 2.0 ** -37))
    assert bool(((back.v.cpu().double().view_as(x64) - x64).abs() <= tol).all()), f'{what}: unpacked image off its reference'


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(SPL)
def test_bias_act_bwd_split_forms(c, mode):
    from rick_amd._lib import lib
    rows, C, N = c.rows, c.C, c.N
    b = build_bab(c, mode)
    # the adjoint has no summation: the fp32 expression in the kernel's association is the fp64 one rounded twice
    o32 = torch.where(b.ref > 0, b.g, b.g * b.alpha) * b.scale
    assert o32.dtype == torch.float32 and bool(((o32.double() - b.o).abs() <= 2 * U * b.o.abs()).all())
    if mode == 'exact':
        assert torch.equal(o32.double(), b.o)
    A = float(b.g.abs().max())
    word = amax_word(A)
    two, cs, f32out = 'out2' in c.form, 'cs' in c.form, 'f32' in c.form
    mul2 = 0.5 if mode == 'exact' else f32(1 / math.sqrt(2))
    g, ref, noise = dev_in(b.g), dev_in(b.ref), dev_in(b.noise)
    img1, hdr1 = Guarded(rows * C), Guarded(4)
    img2, hdr2 = (Guarded(rows * C), Guarded(4)) if two else (None, None)
    out32 = Guarded(rows * C) if f32out else None
    part = Guarded(c.plan.nb * (C + 1))
    gb = Guarded(C) if 'b' in c.want else None
    gnw = Guarded(1) if 'w' in c.want else None
    tail = (p(gb), p(gnw), p(noise), rows, C, c.hw, max(c.noise_nb, 1), c.hw, b.alpha, b.scale, p(part), 0, stream())
    o1_32, o1_64, word1, coef1 = o32, b.o, word, abs(b.scale) * max(1.0, abs(b.alpha))
    if cs:
        s = divisor_for(c, mode)                                          # [N, C]: powers of two, sign-mixed / |normal| + 0.5
        img_of_row = torch.arange(rows) // c.hw
        o1_32, o1_64 = o32 * s[img_of_row], b.o * s.double()[img_of_row]
        # the caller's bound of image 1: |scale| * max |chan_scale| * max |g| (a hair above, against its own rounding)
        word1, coef1 = amax_word(f32(abs(b.scale) * float(s.abs().max()) * A * (1.0 if mode == 'exact' else 1.001))), 1.0
        assert float(o1_32.abs().max()) <= float(word1.v.max())
    if cs or f32out:
        sd = dev_in(s) if cs else None
        rc = lib.rick_bias_act_bwd_split2_f32(p(g), p(ref), p(img1), p(hdr1), p(img2), p(hdr2), mul2 if two else 0.0, p(word), p(sd),
                                              p(word1) if cs else None, p(out32), *tail)
    else:
        rc = lib.rick_bias_act_bwd_split_f32(p(g), p(ref), p(img1), p(hdr1), p(img2), p(hdr2), mul2 if two else 0.0, p(word), *tail)
    assert rc == 0
    torch.cuda.synchronize()
    check_image(c, mode, img1, hdr1, o1_32, o1_64, word1, coef1, 'image 1')
    if two:
        check_image(c, mode, img2, hdr2, b.g * mul2, b.g.double() * mul2, word, abs(mul2), 'image 2')
    if f32out:
        out32.assert_bands(c.id + ' out_f32')
        assert torch.equal(out32.v.cpu().view_as(o32), o32)
        compare(c, mode, out32.v, b.o, b.o.abs(), 1, 1, 'out_f32')
    part.assert_bands(c.id + ' partials')
    check_partials(c, mode, part, b, 'b' in c.want, 'w' in c.want)
    if gb is not None:
        gb.assert_bands(c.id + ' gb')
        compare(c, mode, gb.v, b.gb, b.Sgb, rows, 2, 'gb')
    if gnw is not None:
        gnw.assert_bands(c.id + ' gnw')
        compare(c, mode, gnw.v, b.gnw, b.Sgnw, rows * C, 3, 'gnw')
    cnt = ctypes.c_uint(7)
    assert lib.rick_saturation_count(ctypes.byref(cnt), 0) == 0 and cnt.value == 0


@gpu
def test_split_adjoint_takes_every_multiple_of_four_channels_and_nothing_else():
    """The entry's channel contract is rick_split_pack_f32's, C % 4 == 0 (16 bytes per four channels at the float4's own address:
    the SPL cases at C = 36 hold the image to the standalone pack); the MFMA consumers check their own C % 32.  Other channel
    counts and offset pointers are refused before anything is written."""
    from rick_amd._lib import lib
    rows = 20
    for C, off in ((6, 0), (34, 0), (1, 0), (36, 1)):
        g, ref, img, hdr, word = Guarded(rows * C, off), Guarded(rows * C), Guarded(rows * C), Guarded(4), amax_word(1.0)
        rc = lib.rick_bias_act_bwd_split_f32(p(g), p(ref), p(img), p(hdr), None, None, 0.0, p(word), None, None, None, rows, C, rows, 1, rows,
                                             0.25, 2.0, None, 0, stream())
        torch.cuda.synchronize()
        assert rc == EINVAL and all_sentinel(img, hdr), (C, off)


# ------------------------------------------------------------------------------------------------- GPU: column sums
@gpu
@pytest.mark.parametrize('mode', MODES)
@params(COLSUM)
def test_colsum_forms(c, mode):
    from rick_amd._lib import lib
    assert colsum_plan(c.rows, c.ncols)[2] == c.trips
    b = build_colsum(c.id, mode, c.rows, c.stride, c.ncols, 0, c.acc)
    part, out = dev_in(b.part), out_buf(c.ncols, b.old)
    assert lib.rick_colsum_f32(p(part), p(out), c.rows, c.stride, c.ncols, int(c.acc), stream()) == 0
    torch.cuda.synchronize()
    out.assert_bands(c.id)
    part.assert_bands(c.id + ' partials')
    compare(c, mode, out.v, b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(MULTI)
def test_colsum_multi_forms(c, mode):
    """Every item against fp64, and bit-equal to the single-item launch on the same partial rows (both modes)."""
    from rick_amd._lib import ColsumItem, lib
    specs = multi_items(c.n)
    items = (ColsumItem * c.n)()
    keep = []
    for i, (nb, ncols, pad, col0, split, acc) in enumerate(specs):
        stride = ncols + pad + col0
        b = build_colsum(f'multi/{i}', mode, nb, stride, ncols, col0, acc)
        part = dev_in(b.part)
        n1 = split if split else ncols
        out = out_buf(n1, None if b.old is None else b.old[:n1])
        out2 = out_buf(ncols - split, None if b.old is None else b.old[split:]) if split else None
        single = out_buf(ncols, b.old)
        items[i] = ColsumItem(p(part), p(out), p(out2), nb, stride, ncols, col0, split, acc)
        keep.append((b, part, out, out2, single))
    assert lib.rick_colsum_multi_f32(items, c.n, stream()) == 0
    for (nb, ncols, pad, col0, split, acc), (b, part, out, out2, single) in zip(specs, keep):
        assert lib.rick_colsum_f32(p(part) + 4 * col0, p(single), nb, ncols + pad + col0, ncols, acc, stream()) == 0
    torch.cuda.synchronize()
    for i, ((nb, ncols, pad, col0, split, acc), (b, part, out, out2, single)) in enumerate(zip(specs, keep)):
        ci = case(id=f'{c.id}[{i}: nb{nb} ncols{ncols} col0{col0} split{split} acc{acc}]')
        for g in (out, out2, single):
            if g is not None:
                g.assert_bands(ci.id)
        got = out.v if out2 is None else torch.cat([out.v, out2.v])
        assert torch.equal(got, single.v), f'{ci.id}: differs from the single-item launch'
        compare(ci, mode, got, b.ref, b.S, b.n, b.k)


@gpu
def test_colsum_multi_rejects_a_bad_item_before_any_launch():
    from rick_amd._lib import ColsumItem, lib
    part, out = Guarded(64), Guarded(8)
    items = (ColsumItem * 2)(ColsumItem(p(part), p(out), None, 4, 8, 8, 0, 0, 0), ColsumItem(p(part), p(out), None, 4, 4, 8, 0, 0, 0))
    assert lib.rick_colsum_multi_f32(items, 2, stream()) == EINVAL and lib.rick_colsum_multi_f32(items, 0, stream()) == EINVAL
    assert lib.rick_colsum_f32(p(part), p(out), 4, 4, 8, 0, stream()) == EINVAL
    torch.cuda.synchronize()
    assert all_sentinel(out)


# ---------------------------------------------------------------------------------------------------- GPU: the forward
@gpu
@pytest.mark.parametrize('mode', MODES)
@params(FWD)
def test_bias_act_fwd_forms(c, mode):
    from rick_amd._lib import lib
    b = build_fwd(c, mode)
    x, bias, noise, nw, ref = dev_in(b.x, c.ox), dev_in(b.bias), dev_in(b.noise), dev_in(b.nw), dev_in(b.ref_in, c.oref)
    out = out_buf(c.n, off=c.oout)
    rc = lib.rick_bias_act_f32(p(x), p(bias), p(ref), p(out), c.n, c.step_b, c.C, b.act, b.grad, b.alpha, b.scale, p(noise), p(nw),
                               c.n_div, c.hw_div, max(c.noise_nb, 1), c.HW, stream())
    assert rc == 0
    torch.cuda.synchronize()
    out.assert_bands(c.id)
    compare(c, mode, out.v, b.ref, b.S, b.n, b.k)
