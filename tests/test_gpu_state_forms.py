"""The small kernels that run between the layers on every training step, through the C ABI, against the fp64 expressions and the
byte-level split-image model of tests/state_f64.py: rick_split_pack_f32 / rick_split_unpack_f32, rick_amax_f32, rick_bound_tail_f32
(rick_amd/csrc/split.hip); rick_add_scale_split_f32, rick_masked_adam_f32 / rick_masked_adam_dev_f32 / rick_adam_prepare_f32,
rick_ema_f32, rick_sq_accumulate_f32, rick_filter_reduce_f32, rick_mbstd_{fwd,bwd}_f32 (rick_amd/csrc/elementwise.hip);
rick_image_batch_f32 (rick_amd/csrc/data.hip).  The method is that of tests/test_gpu_mod_forms.py; tests/forms_common.py holds what
the forms files share.

No tolerance here was read off the device:
  exact   small sign-mixed integers and power-of-two coefficients: the device result must be torch.equal to the fp64 result cast
          to fp32 (the CPU asserts before the launch that it is an fp32 number).  rick_amax_f32, rick_bound_tail_f32 and
          rick_image_batch_f32 are exact by nature: the whole amax word is predicted per block and slot, the image batch is held to
          a 256-entry table evaluated in fp32 on the CPU.
  bound   operands from rick_amd.synth; per element |dev - ref64| <= k * 2**-24 * sum |terms| + one ulp of the result, k counted
          next to each check (one rounding per written operation, two for a division or a sqrtf).
  split images are compared BYTE FOR BYTE with the host model (numpy and torch fp16 conversions, which agree), the header with the
          exponent rule replayed in integer arithmetic, its three clamps included; the data are arbitrary fp32 values: at the bound,
          2^-10 and 2^-20 of it (subnormal and zero `lo` halves), +-0, both signs.
  masked Adam   m and v against fp64 (k = 4: g - m, 1 - beta1, the product, the sum; k = 5: v beta2, 1 - beta2, two products, the
          sum); p against the update evaluated in fp64 from the moments the device wrote, 14 * 2**-24 |update| + one ulp: lr / bc1
          (2), 1 / sqrtf(bc2) (4), sqrtf(v) (2), the product (1), + eps (1), m / denom (2), the product with the step (1), and one
          for the second-order terms.  In exact mode m and v are torch.equal; the three steps of bound mode each start from the
          device's own state, so no error is carried from step to step into a bound.
  minibatch stddev   stat: the bound derived in state_f64.mbstd_stat_bound; gx (x - mean cancels): four times the error of the
          fp32 CPU composition of the same formula against the same fp64 reference, largest element against
          largest element, per shape; both figures are printed with -s.  Without a tolerance: the copy of x, channel C against
          stat[g] bit for bit, gs = 1, and a grouped call against the separate calls.

Around every launch: outputs and in-place buffers lie between sentinel bands that stay intact; read-only operands are views with a
fence on both sides: NaN for floats, +inf where the operand only passes through fmaxf (which drops a NaN: the data of
rick_amax_f32, the bias and mul of rick_bound_tail_f32, the floats between the 16 slots of every amax word a kernel reads), 0xFF
bytes for masks, flips and source images, the index of a NaN-free decoy image (never sampled by a case) for `index`.  Flat-buffer
operands (p, g, m, v, ema, acc) start one float off a 16-byte boundary.  rick_saturation_count stays put in every test but the one
about it.  Every RICK_EINVAL written in the entry points returns with nothing written, and so does every zero-size call (rc 0).

rick_saturation_count counts threads whose largest scaled value reaches the end of the fp16 range (|v| 2^e >= 65504, cv_sat_check):
the case about it plants a value 16 times the bound, where hi itself would clamp; a value a little above the bound is still
represented exactly and is not an event.

The case builders and the launcher replays are host-only (test_case_tables_reach_every_form_and_stay_exact).

What these cases caught when one line of a scratch copy of the sources was changed.  The six changes lie in six different
kernels and every test here launches one kernel family, so they were built into ONE scratch library and this file was run
against it once on an MI355X (116 red, 153 green); each of them changes values or in-fence indices only:
  amax_kernel             the scalar tail dropped            test_amax_forms[1|2|3|5|7|1023|24581], 7 of 10 (n % 4 == 0 has no tail and
                                                             stays green; at 5, 7, 1023 and 24581 only the launches with the
                                                             maximum in the tail differ)
  cv_split_store4         hi and lo halves swapped           all 15 of test_split_pack_forms, the saturation test's byte check and all
                                                             10 of test_add_scale_split_forms (its image against the host model;
                                                             against rick_split_pack_f32 alone it stayed green: both were swapped
                                                             alike, which is why the host model is asked there too);
                                                             rick_split_unpack_f32 does not use it: 15 green
  masked_adam_kernel      mk & 2 -> mk & 1                   test_masked_adam_forms[*-mask-*], all 10, and all 4 of
                                                             test_masked_adam_dev_reads_the_prepared_corrections; mask = NULL stays green
  filter_reduce_kernel    outer_stride ignored               test_filter_reduce_forms[outer3-*], all 60; outer = 1 stays green
  mbstd_fwd_kernel        copy loop i += 2048                6 of 7 test_mbstd_forms (the sentinel is left in out); B3-groups3-P1-C3
                                                             writes 4 floats in the first pass and stays green
  image_batch_kernel      flip ignored                       all 3 of test_image_batch_forms
"""
import ctypes
import functools
import math
import types

import numpy as np
import pytest
import torch

from rick_amd.synth import synth_tensor
from tests import state_f64 as R
from tests.forms_common import (AMAX_FLOATS, AMAX_STRIDE, DEV, Fenced, Guarded, amax_word_check, cdiv, f32, fenced, ints, p, sat_count,
                                stream)

gpu = pytest.mark.gpu
U = 2.0 ** -24
MODES = ('exact', 'bound')
EINVAL = 22
INF = float('inf')
EW_BLOCKS = 4096                         # ew_grid's cap: 4096 blocks of 256 threads, grid-stride beyond
N_LIST = (1, 255, 257, 100003, (1 << 20) + 257)
BIG = (1 << 20) + 3
LR, BETA1, BETA2, ADAM_EPS = f32(0.002 * 0.8), 0.0, f32(0.99 ** 0.8), f32(1e-8)         # the trainer's optimisers
EMA_DECAY = f32(0.5 ** (32 / (10 * 1000)))                                                # TrainConfig.ema_decay: 0.997784


def case(**kw):
    return types.SimpleNamespace(**kw)


def params(cases):
    return pytest.mark.parametrize('c', cases, ids=[c.id for c in cases])


def key(*parts):
    return 'stateforms/' + '/'.join(str(x) for x in parts)


# ------------------------------------------------------------------------------------------ host-side launcher replay
def trips(n, blocks):
    """A grid-stride loop of `blocks` x 256 threads over n items -> (fewest, most) passes of a thread."""
    t = blocks * 256
    return n // t, cdiv(n, t)


def ew_blocks(n):
    return max(min(cdiv(n, 256), EW_BLOCKS), 1)


def split_blocks(n4):
    return max(min(cdiv(n4, 256 * 8), 8192), 1)


def amax_blocks(n):
    return max(min(cdiv(n >> 2, 256 * 8), 2048), 1)


def amax_block_of(n):
    """amax_kernel: the block every element is read by (float4 i by block (i mod blocks * 256) / 256, the scalar tail by block 0)."""
    nb, n4 = amax_blocks(n), n >> 2
    blk = (np.arange(n4 * 4) // 4 % (nb * 256)) // 256
    return np.concatenate([blk, np.zeros(n - n4 * 4, dtype=blk.dtype)]), nb


def amax_positions(n):
    """Where the maximum is planted: element 0, the last full float4, every scalar tail element, and the last float4 a later pass
    reads -> sorted list."""
    n4, nb = n >> 2, amax_blocks(n)
    pos = {0} | set(range(n4 * 4, n))
    if n4:
        pos.add(n4 * 4 - 2)
    if n4 > nb * 256:
        pos.add((nb * 256 + (n4 - nb * 256) // 2) * 4 + 1)
    return sorted(pos)


def amax_expected_word(x, pre):
    """The whole word after rick_amax_f32: block b folds its maximum into slot b mod 16."""
    blk, nb = amax_block_of(x.numel())
    out, a = pre.clone(), x.abs().numpy()
    for b in range(nb):
        s = (b & 15) * AMAX_STRIDE
        out[s] = max(float(out[s]), float(a[blk == b].max()) if bool((blk == b).any()) else 0.0)
    return out


def filter_idle_waves(nfilters):
    return cdiv(nfilters, 4) * 4 - nfilters


def mbstd_forms(B, groups, P, C):
    """mbstd kernels, 1024 threads per run: (passes of the statistics loop, passes of the copy loop, passes of the G loop)."""
    gs = B // groups
    return trips(P * C, 4), trips(gs * P * (C + 1), 4), trips(gs * P, 4)


def image_blocks(B, H, W):
    return min(cdiv(B * H * W, 256), 65535)


# ------------------------------------------------------------------------------------------------------------ inputs
def fill(k, shape, mode, amp):
    return synth_tensor(k, shape) if mode == 'bound' else ints(k, shape, amp)


def word(value, slot, between=INF):
    """An amax word a kernel only reads: `value` in `slot`, smaller non-negative values in the other 15, `between` elsewhere."""
    w = torch.full((AMAX_FLOATS,), between)
    for s in range(16):
        w[s * AMAX_STRIDE] = float(np.float32(value) * np.float32((1 + (s * 7) % 16) / 32))
    w[slot * AMAX_STRIDE] = value
    assert float(R.amax_read(w.numpy())) == float(np.float32(value))
    return w


def ulp32(ref):
    """One ulp of ref cast to fp32, per element (fp64)."""
    _, e = torch.frexp(ref.float())
    return 2.0 ** (e.double() - 24)


def is_f32(t):
    return torch.equal(t.float().double(), t)


# ------------------------------------------------------------------------------------------------------- split images
def pack_values(k, n, bound, coarse=False):
    """Arbitrary fp32 data with |v| <= bound.  fine: thirds at full scale, 2^-10 and 2^-20 of it, with +-bound, bound 2^-10,
    bound 2^-20 and +-0 planted; coarse (the tiny bounds: no input may be an fp32 subnormal): +-bound (8 + j) / 16."""
    bound = np.float32(bound)
    t = synth_tensor(k, (n,)).numpy()
    if coarse:
        v = np.sign(t) * bound * ((8 + np.arange(n) % 9) / 16).astype(np.float32)
        v[n // 2] = bound
        return v.astype(np.float32)
    u = t / np.abs(t).max()
    v = (u * bound * (np.float32(2.0) ** (-10 * (np.arange(n) % 3))).astype(np.float32)).astype(np.float32)
    plant = [bound, -bound * np.float32(2.0 ** -10), np.float32(-0.0), bound * np.float32(2.0 ** -20), -bound, np.float32(0.0),
             bound * np.float32(2.0 ** -10), -bound * np.float32(2.0 ** -20)]
    for j, pos in enumerate(np.linspace(0, n - 1, len(plant)).astype(int) if n >= len(plant) else range(n)):
        v[pos] = plant[j]
    assert float(np.abs(v).max()) == float(bound)
    return v


PACK_SHAPES = [case(id=f'n4_{npix * C // 4}-C{C}', npix=npix, C=C) for npix, C in
               ((1, 4), (255, 4), (256, 4), (257, 4), (3 * 2048 + 5, 4), (1, 36), (29, 36), (683, 36))]
# a0 / a1: (maximum, slot); clamp: which clamp of the exponent rule acts
PACK_HEADERS = [case(id='sum-coef0.7071', a0=(5.3, 5), a1=(2.9, 11), coef=f32(0.7071), clamp=None),
                case(id='a0-pow2', a0=(8.0, 3), a1=None, coef=1.0, clamp=None),
                case(id='a0-ones-mantissa', a0=(float(np.nextafter(np.float32(16), np.float32(0))), 15), a1=None, coef=1.0, clamp=None),
                case(id='sum-coef3', a0=(1.1, 1), a1=(0.3, 2), coef=3.0, clamp=None),
                case(id='edge-2^-113', a0=(2.0 ** -113, 4), a1=None, coef=1.0, clamp=None),
                case(id='clamp-zero', a0=(0.0, 6), a1=(0.0, 8), coef=f32(0.7071), clamp='zero'),
                case(id='clamp-low', a0=(2.0 ** -120, 7), a1=None, coef=1.0, clamp='low'),
                case(id='clamp-high', a0=(2.0 ** 127, 9), a1=None, coef=1.0, clamp='high')]
PACK_RUNS = [(s, PACK_HEADERS[0]) for s in PACK_SHAPES] + [(PACK_SHAPES[3], h) for h in PACK_HEADERS[1:]]
PACK_IDS = [f'{s.id}-{h.id}' for s, h in PACK_RUNS]


def build_pack(s, h):
    n = s.npix * s.C
    w0 = word(f32(h.a0[0]), h.a0[1])
    w1 = word(f32(h.a1[0]), h.a1[1]) if h.a1 else None
    hdr, clamp = R.split_header(w0.numpy(), w1.numpy() if h.a1 else None, h.coef)
    assert clamp == h.clamp and h.a0[1] != 0 and float(hdr[0]) * float(hdr[1]) == 1.0
    if clamp is None:
        assert 2.0 ** 13 <= float(hdr[2]) * float(hdr[0]) < 2.0 ** 14, 'an ordinary bound is placed in [2^13, 2^14)'
    # a zero bound splits raw values (2^e = 1): modest ones, so nothing saturates
    coarse = 0 < float(hdr[2]) < 2.0 ** -90
    x = pack_values(key('pack', s.id, h.id), n, hdr[2] if clamp != 'zero' else 4.0, coarse)
    assert bool(np.isfinite(x).all()) and (n < 8 or (bool((x > 0).any()) and bool((x < 0).any())))
    assert bool((np.abs(x[x != 0]) >= 2.0 ** -126).all()), 'an fp32 subnormal input'
    img = R.split_image(x, hdr[0])
    hi, lo = R.split_halves_of(img)
    assert bool(np.isfinite(hi.astype(np.float32)).all()) and bool(np.isfinite(lo.astype(np.float32)).all())
    if n >= 1000 and clamp is None and not coarse:
        lob = lo.view(np.uint16) & 0x7FFF
        assert bool(((lob > 0) & (lob < 0x0400)).any()) and bool((lob == 0).any()) and bool((lob >= 0x0400).any()), 'no subnormal / zero / normal lo'
        assert bool((hi.view(np.uint16) == 0x8000).any()) and bool((hi.view(np.uint16) == 0).any()), 'no -0 / +0'
    return case(x=x, w0=w0, w1=w1, hdr=hdr, img=img, n=n)


def words_on_device(*ws):
    return [fenced(w, fill=INF) for w in ws]


def same_bytes(got, exp, what):
    got, exp = np.asarray(got).reshape(-1), np.asarray(exp).reshape(-1)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f'{what}: {bad.size} of {got.size} bytes differ, first in value {bad[0] // 16 * 4 + bad[0] % 8 // 2} ({"lo" if bad[0] % 16 >= 8 else "hi"} half)'


def same_bits(a, b, what):
    a, b = a.detach().reshape(-1), b.detach().reshape(-1).to(a.device)
    assert a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: the bit patterns differ'


class FencedInts:
    """A read-only uint8 / integer operand with `fence` in every element either side of it."""

    def __init__(self, src, fence, pad=64):
        src = src.reshape(-1)
        self.buf = torch.full((pad + src.numel() + pad,), fence, dtype=src.dtype, device=DEV)
        self.v = self.buf[pad:pad + src.numel()]
        self.v.copy_(src)


def ok(rc, what):
    assert rc == 0, f'{what}: rc = {rc}'
    torch.cuda.synchronize()


def steady(fn):
    """rick_saturation_count is where it was when the test ends."""
    @functools.wraps(fn)
    def run(*a, **kw):
        before = sat_count()
        fn(*a, **kw)
        assert sat_count() == before, 'a saturation event was counted'
    return run


def within(cid, got, ref, bound, what):
    got = got.detach().cpu().reshape(ref.shape)
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f'{cid} {what}: max |err| / bound = {worst:.3f}')
    assert bool((err <= bound).all()), f'{cid} {what}: |err| up to {worst:.3f} x the a-priori bound'


def equal64(cid, got, ref, what):
    got, exp = got.detach().cpu().reshape(ref.shape), ref.float()
    bad = got != exp
    assert not bool(bad.any()), (f'{cid} {what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {tuple(bad.nonzero()[0].tolist())}: '
                                 f'{float(got[bad][0])} != {float(exp[bad][0])}')


def compare(cid, mode, got, ref, S, k, what='out'):
    if mode == 'exact':
        equal64(cid, got, ref, what)
    else:
        within(cid, got, ref, k * U * S + ulp32(ref), what)


def run_pack(x, w0, w1, coef, npix, C, what):
    """-> (image bytes, header) on the CPU"""
    from rick_amd._lib import lib
    n = npix * C
    src, (a0, a1) = fenced(torch.from_numpy(np.ascontiguousarray(x))), words_on_device(w0, w1)
    img, hdr = Guarded(n), Guarded(4)
    ok(lib.rick_split_pack_f32(p(src), p(img), p(hdr), p(a0), p(a1), coef, npix, C, stream()), what)
    img.assert_bands(what)
    hdr.assert_bands(what)
    return img.v.cpu().numpy().view(np.uint8), hdr.v.cpu().numpy()


@gpu
@pytest.mark.parametrize('s,h', PACK_RUNS, ids=PACK_IDS)
@steady
def test_split_pack_forms(s, h):
    b = build_pack(s, h)
    img, hdr = run_pack(b.x, b.w0, b.w1, h.coef, s.npix, s.C, f'{s.id}-{h.id}')
    assert np.array_equal(hdr.view(np.uint32), b.hdr.view(np.uint32)), f'header {hdr.tolist()} != {b.hdr.tolist()}'
    same_bytes(img, b.img, 'image against the host model')


@gpu
@pytest.mark.parametrize('s,h', PACK_RUNS, ids=PACK_IDS)
@steady
def test_split_unpack_forms(s, h):
    """The host model's image (fp16 NaN on both sides) -> (hi + lo) * 2^-e bit for bit; the round trip keeps 2^-22 relative for
    |v| >= 2^-10 of the bound (include/rick_hip.h)."""
    from rick_amd._lib import lib
    b = build_pack(s, h)
    img, hdr, out = Fenced(b.n, image=True), fenced(torch.from_numpy(b.hdr)), Guarded(b.n)
    img.v.view(torch.uint8).copy_(torch.from_numpy(b.img))
    ok(lib.rick_split_unpack_f32(p(img), p(hdr), p(out), s.npix, s.C, stream()), 'unpack')
    out.assert_bands('unpack')
    got, exp = out.v.cpu().numpy(), R.split_decode(b.img, b.hdr[1])
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), f'{int((got.view(np.uint32) != exp.view(np.uint32)).sum())} of {b.n} values differ'
    if h.clamp is None:
        x64, big = b.x.astype(np.float64), np.abs(b.x) >= 2.0 ** -10 * float(b.hdr[2])
        assert bool(big.any()) and bool((np.abs(got.astype(np.float64) - x64)[big] <= 2.0 ** -22 * np.abs(x64)[big]).all())


@gpu
@pytest.mark.saturates
def test_split_pack_counts_a_value_that_saturates():
    """One value 16 times the bound: hi would clamp, one thread reports it; every other float4 is still the host model's."""
    from rick_amd._lib import check, lib
    s, h = PACK_SHAPES[3], PACK_HEADERS[0]
    b = build_pack(s, h)
    x = b.x.copy()
    x[4 * 100 + 1] = 16 * b.hdr[2]
    assert float(x[401]) * float(b.hdr[0]) >= 65504
    before = sat_count()
    try:
        img, hdr = run_pack(x, b.w0, b.w1, h.coef, s.npix, s.C, 'saturating pack')
        assert sat_count() == before + 1
    finally:
        cnt = ctypes.c_uint(0)
        check(lib.rick_saturation_count(ctypes.byref(cnt), 1), 'reset')
    assert cnt.value == before + 1 and sat_count() == 0
    keep = np.ones(b.n * 4, dtype=bool)
    keep[16 * 100:16 * 101] = False
    same_bytes(img[keep], b.img[keep], 'the other values')


# ------------------------------------------------------------------------------------------- rick_add_scale_split_f32
ASS = [case(id=f'n4_{rows * C // 4}-C{C}', rows=rows, C=C) for rows, C in ((1, 4), (257, 4), (BIG, 4), (1, 36), (17, 64))]


def build_ass(c, mode):
    """(a + b) and the product: 2 roundings."""
    n = c.rows * c.C
    a, b = fill(key('ass', c.id, 'a'), (n,), mode, 50), fill(key('ass', c.id, 'b'), (n,), mode, 50)
    alpha = -0.5 if mode == 'exact' else -f32(0.7071)
    ref, S = R.add_scale(a, b, alpha)
    if mode == 'exact':
        assert is_f32(ref)
    assert n < 64 or (float(ref.min()) < 0 < float(ref.max()))
    return case(a=a, b=b, alpha=alpha, ref=ref, S=S, n=n, wa=word(float(a.abs().max()), 13), wb=word(float(b.abs().max()), 2))


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(ASS)
@steady
def test_add_scale_split_forms(c, mode):
    from rick_amd._lib import lib
    b = build_ass(c, mode)
    a_, b_, (wa, wb) = fenced(b.a), fenced(b.b), words_on_device(b.wa, b.wb)
    y, img, hdr = Guarded(b.n), Guarded(b.n), Guarded(4)
    ok(lib.rick_add_scale_split_f32(p(a_), p(b_), p(y), p(img), p(hdr), p(wa), p(wb), c.rows, c.C, b.alpha, stream()), c.id)
    for gd in (y, img, hdr):
        gd.assert_bands(c.id)
    compare('add-scale-split-' + c.id, mode, y.v, b.ref, b.S, 2, 'y')
    # the image and header are those of rick_split_pack_f32 of the y the device wrote, under the same words and coef = |alpha|
    src, img2, hdr2 = Fenced(b.n), Guarded(b.n), Guarded(4)
    src.v.copy_(y.v)
    ok(lib.rick_split_pack_f32(p(src), p(img2), p(hdr2), p(wa), p(wb), abs(b.alpha), c.rows, c.C, stream()), c.id + ' pack')
    same_bits(hdr.v[:3], hdr2.v[:3], 'header')
    same_bits(img.v, img2.v, 'image against rick_split_pack_f32 of y')
    # ... and those of the host model
    exp, _ = R.split_header(b.wa.numpy(), b.wb.numpy(), abs(b.alpha))
    assert np.array_equal(hdr.v.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    same_bytes(img.v.cpu().numpy().view(np.uint8), R.split_image(y.v.cpu().numpy(), exp[0]), 'image against the host model')


# ------------------------------------------------------------------------------------------------------ rick_amax_f32
AMAX_N = (1, 2, 3, 4, 5, 7, 1023, 8 * 256 * 4, 8 * 256 * 4 + 4, 3 * 8192 + 5)
AMAX_MAX = 1000.5


def build_amax(n, pos, sign):
    x = ints(key('amax', n), (n,), 9)
    x[pos] = sign * AMAX_MAX
    return x


def run_amax(x, pre, what):
    from rick_amd._lib import lib
    src, wd = fenced(x, fill=INF), Guarded(AMAX_FLOATS, pre)
    ok(lib.rick_amax_f32(p(src), x.numel(), p(wd), stream()), what)
    wd.assert_bands(what)
    return wd.v.cpu()


@gpu
@pytest.mark.parametrize('n', AMAX_N)
@steady
def test_amax_forms(n):
    for j, pos in enumerate(amax_positions(n)):
        x = build_amax(n, pos, -1.0 if j % 2 else 1.0)
        got = run_amax(x, torch.zeros(AMAX_FLOATS), f'n = {n}, maximum at {pos}')
        amax_word_check(got, AMAX_MAX, f'n = {n}, maximum at {pos}')
        assert torch.equal(got, amax_expected_word(x, torch.zeros(AMAX_FLOATS))), f'n = {n}, maximum at {pos}: a slot is not its blocks\' maximum'


@gpu
@steady
def test_amax_folds_into_a_loaded_word():
    n = 8 * 256 * 4 + 4
    x = build_amax(n, n - 1, -1.0)
    larger = torch.zeros(AMAX_FLOATS)
    larger[::AMAX_STRIDE] = 2000.0
    got = run_amax(x, larger, 'larger')
    amax_word_check(got, 2000.0, 'a word holding a larger value')
    assert torch.equal(got, larger)
    smaller = torch.zeros(AMAX_FLOATS)
    smaller[::AMAX_STRIDE] = 1.0
    got = run_amax(x, smaller, 'smaller')
    amax_word_check(got, AMAX_MAX, 'a word holding a smaller value')
    assert torch.equal(got, amax_expected_word(x, smaller)) and float(got[::AMAX_STRIDE].min()) == 1.0


# ------------------------------------------------------------------------------------------------ rick_bound_tail_f32
BT_SIZES = (1, 255, 256, 257, 700)
BT_TERMS = [(n, b, m) for n in ('', 'nw+noise') for b in (0, 1) for m in (0, 1)] + [('nw', 1, 1), ('noise', 1, 1)]
BOUND_TAIL = [case(id=f'{t[0] or "plain"}{"-bias" if t[1] else ""}{"-mul" if t[2] else ""}-nb{BT_SIZES[j % 5]}-nm{BT_SIZES[(2 * j + 1) % 5]}',
                   noise=t[0], bias=t[1], mul=t[2], nbias=BT_SIZES[j % 5], nmul=BT_SIZES[(2 * j + 1) % 5]) for j, t in enumerate(BT_TERMS)]
BOUND_TAIL += [case(id=f'all-nb{nb}-nm{nm}', noise='nw+noise', bias=1, mul=1, nbias=nb, nmul=nm) for nb in BT_SIZES for nm in BT_SIZES]


def build_bound_tail(c):
    """Powers of two and small integers: every product and sum is an exact small integer.  The maxima of bias and mul are their
    last elements and negative."""
    bias = ints(key('bt', c.id, 'bias'), (c.nbias,), 9)
    bias[-1] = -16.0
    mul = ints(key('bt', c.id, 'mul'), (c.nmul,), 3)
    mul[-1] = -4.0
    b = case(w0=word(8.0, 10), c0=0.5, gain=2.0, nw=torch.tensor([-2.0]) if 'nw' in c.noise else None,
             noise=word(4.0, 14) if 'noise' in c.noise else None, bias=bias if c.bias else None, mul=mul if c.mul else None)
    b.ref = R.bound_tail(8.0, b.c0, -2.0 if b.nw is not None else None, 4.0 if b.noise is not None else None, b.bias, b.gain, b.mul)
    assert b.ref == (4 if c.mul else 1) * 2 * (4 + (16 if c.bias else 0) + (8 if c.noise == 'nw+noise' else 0))
    return b


@gpu
@params(BOUND_TAIL)
@steady
def test_bound_tail_forms(c):
    from rick_amd._lib import lib
    b = build_bound_tail(c)
    (w0, noise), nw = words_on_device(b.w0, b.noise), fenced(b.nw)
    bias, mul, out = fenced(b.bias, fill=INF), fenced(b.mul, fill=INF), Guarded(AMAX_FLOATS)
    # a NULL bias / mul comes with a non-zero count: the entry point must not pass it on
    ok(lib.rick_bound_tail_f32(p(out), p(w0), b.c0, p(nw), p(noise), p(bias), c.nbias, b.gain, p(mul), c.nmul, stream()), c.id)
    out.assert_bands(c.id)
    got = out.v.cpu()
    assert float(got[0]) == b.ref, f'{c.id}: {float(got[0])} != {b.ref}'
    assert not bool(got[1:].any()), f'{c.id}: the other 511 floats are not zero'


# ------------------------------------------------------------------------------------------------------ masked Adam
ADAM = [case(id=f'n{n}-{"mask" if mk else "nomask"}', n=n, mask=mk) for n in N_LIST for mk in (1, 0)]
ADAM_EXACT = case(lr=2.0 ** -6, beta1=0.5, beta2=0.75, eps=2.0 ** -10, bc=[(0.5, 0.25)])
ADAM_REAL = case(lr=LR, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, bc=[(f32(1 - BETA1 ** t), f32(1 - BETA2 ** t)) for t in (1, 2, 3)])


def adam_mask(c):
    if not c.mask:
        return None
    gen = torch.Generator().manual_seed(c.n)
    mask = torch.randint(0, 4, (c.n,), generator=gen).to(torch.uint8)
    mask[0] = 2
    assert c.n < 255 or set(mask.tolist()) == {0, 1, 2, 3}
    return mask


def adam_state(c, mode):
    """Non-zero m and v.  exact: g integer, m even, v a positive multiple of 4."""
    k = key('adam', c.id)
    if mode == 'exact':
        return ints(k + 'p', (c.n,), 9), 2 * ints(k + 'm', (c.n,), 5), 4 * ints(k + 'v', (c.n,), 6).abs()
    return synth_tensor(k + 'p', (c.n,)), 0.1 * synth_tensor(k + 'm', (c.n,)), (0.1 * synth_tensor(k + 'v', (c.n,))) ** 2 + f32(1e-4)


def adam_grad(c, mode, step):
    return fill(key('adam', c.id, 'g', step), (c.n,), mode, 7)


def adam_expect(h, p0, g0, m0, v0, mask, mode):
    pp, gm, mn, Sm, vn, Sv = R.masked_adam_moments(p0, g0, m0, v0, mask, h.beta1, h.beta2)
    if mode == 'exact':
        assert is_f32(mn) and is_f32(vn) and is_f32(gm - m0.double()) and bool((vn > 0).all()) and bool((mn != m0.double()).any())
        if mask is not None:            # a pruned parameter still drifts by its momentum: the order "prune, then update" is visible
            assert bool((mn[(mask & 2) != 0] != 0).all())
    return case(pp=pp, g=gm.float(), m=mn, Sm=Sm, v=vn, Sv=Sv)


def adam_check(cid, mode, h, bc, e, p1, g1, m1, v1):
    same_bits(g1, e.g, f'{cid}: g (kept where unmasked, +0 where masked)')
    compare(cid, mode, m1, e.m, e.Sm, 4, 'm')
    compare(cid, mode, v1, e.v, e.Sv, 5, 'v')
    ref, t = R.adam_update(e.pp, m1, v1, h.lr, h.eps, bc[0], bc[1])
    within(cid, p1, ref, 14 * U * t + ulp32(ref), 'p')
    assert p1.numel() == 1 or bool((t > 0).any())


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(ADAM)
@steady
def test_masked_adam_forms(c, mode):
    from rick_amd._lib import lib
    h = ADAM_EXACT if mode == 'exact' else ADAM_REAL
    mask = adam_mask(c)
    p0, m0, v0 = adam_state(c, mode)
    pd, md, vd = Guarded(c.n, p0, off=1), Guarded(c.n, m0, off=1), Guarded(c.n, v0, off=1)
    mk = FencedInts(mask, 0xFF) if c.mask else None
    for step, bc in enumerate(h.bc, 1):
        g0 = adam_grad(c, mode, step)
        e = adam_expect(h, p0, g0, m0, v0, mask, mode)
        gd = Guarded(c.n, g0, off=1)
        ok(lib.rick_masked_adam_f32(p(pd), p(gd), p(md), p(vd), p(mk), c.n, h.lr, h.beta1, h.beta2, h.eps, bc[0], bc[1], stream()), c.id)
        for b in (pd, gd, md, vd):
            b.assert_bands(c.id)
        p0, m0, v0 = pd.v.cpu(), md.v.cpu(), vd.v.cpu()
        adam_check(f'adam-{c.id}-{mode} step {step}', mode, h, bc, e, p0, gd.v.cpu(), m0, v0)


ADAM_DEV = [case(id=f'n{n}-{name}', n=n, mask=1, h=h) for n in (257, 100003) for name, h in (('pow2', ADAM_EXACT), ('trainer', ADAM_REAL))]


@gpu
@params(ADAM_DEV)
@steady
def test_masked_adam_dev_reads_the_prepared_corrections(c):
    """rick_adam_prepare_f32 -> bc; rick_masked_adam_dev_f32 reading it is bit-equal to rick_masked_adam_f32 given the same two
    floats, and both hold against fp64."""
    from rick_amd._lib import lib
    h, mode = c.h, 'bound'
    mask = adam_mask(c)
    p0, m0, v0 = adam_state(c, mode)
    g0 = adam_grad(c, mode, 1)
    steps = FencedInts(torch.tensor([9, 2, 2, 2, 9], dtype=torch.int32), -77)
    bc = Guarded(2)
    ok(lib.rick_adam_prepare_f32(steps.v.data_ptr(), 1, 3, h.beta1, h.beta2, p(bc), stream()), c.id)
    bc1, bc2 = bc.v.cpu().tolist()
    got = []
    for dev in (1, 0):
        pd, gd, md, vd = Guarded(c.n, p0, off=1), Guarded(c.n, g0, off=1), Guarded(c.n, m0, off=1), Guarded(c.n, v0, off=1)
        mk, bcd = FencedInts(mask, 0xFF), fenced(torch.tensor([bc1, bc2]))
        if dev:
            ok(lib.rick_masked_adam_dev_f32(p(pd), p(gd), p(md), p(vd), p(mk), c.n, h.lr, h.beta1, h.beta2, h.eps, p(bcd), stream()), c.id)
        else:
            ok(lib.rick_masked_adam_f32(p(pd), p(gd), p(md), p(vd), p(mk), c.n, h.lr, h.beta1, h.beta2, h.eps, bc1, bc2, stream()), c.id)
        for b in (pd, gd, md, vd):
            b.assert_bands(c.id)
        got.append([b.v.cpu() for b in (pd, gd, md, vd)])
    for a, b, name in zip(got[0], got[1], 'pgmv'):
        same_bits(a, b, f'{c.id}: {name} of the _dev entry against rick_masked_adam_f32')
    e = adam_expect(h, p0, g0, m0, v0, mask, mode)
    adam_check(f'adam-dev-{c.id}', mode, h, (bc1, bc2), e, *got[0])


PREPARE = [case(id=f'count{n}', count=n) for n in (1, 255, 256, 257, 600)]


@gpu
@params(PREPARE)
def test_adam_prepare_forms(c):
    """steps[first .. first + count) += 1, the neighbours untouched; bc within one fp32 ulp of 1 - beta^t in fp64 from the
    fp32-rounded betas; two calls in a row give t and t + 1."""
    from rick_amd._lib import lib
    first, t0, b1, b2 = 3, 4, f32(0.9), BETA2
    init = torch.arange(1000, 1000 + first + c.count + 5, dtype=torch.int32)
    init[first:first + c.count] = t0
    steps, bc = FencedInts(init, -77), Guarded(2)
    for t in (t0 + 1, t0 + 2):
        ok(lib.rick_adam_prepare_f32(steps.v.data_ptr(), first, c.count, b1, b2, p(bc), stream()), c.id)
        bc.assert_bands(c.id)
        exp = init.clone()
        exp[first:first + c.count] = t
        assert torch.equal(steps.v.cpu(), exp) and bool((steps.buf[:64] == -77).all()) and bool((steps.buf[64 + init.numel():] == -77).all())
        ref = torch.tensor([1 - b1 ** t, 1 - b2 ** t], dtype=torch.float64)
        within(f'prepare-{c.id} t = {t}', bc.v, ref, ulp32(ref), 'bc')


# ------------------------------------------------------------------------------------------ EMA, Fisher accumulation
FLAT = [case(id=f'n{n}', n=n) for n in N_LIST]


def build_ema(c, mode):
    """e decay, 1 - decay, p (1 - decay), the sum: k = 4."""
    e, pp = fill(key('ema', c.id, 'e'), (c.n,), mode, 9), fill(key('ema', c.id, 'p'), (c.n,), mode, 9)
    if mode == 'exact':
        e, pp = 4 * e, 4 * pp
    decay = 0.75 if mode == 'exact' else EMA_DECAY
    ref, S = R.ema(e, pp, decay)
    assert mode == 'bound' or (is_f32(ref) and is_f32(e.double() * decay) and is_f32(pp.double() * (1.0 - decay)))
    assert bool((ref.float() != e).any()) and (mode == 'exact' or abs(decay - 0.997784) < 1e-6)
    return case(e=e, p=pp, decay=decay, ref=ref, S=S)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(FLAT)
@steady
def test_ema_forms(c, mode):
    from rick_amd._lib import lib
    b = build_ema(c, mode)
    e, pp = Guarded(c.n, b.e, off=1), fenced(b.p, off=1)
    ok(lib.rick_ema_f32(p(e), p(pp), c.n, b.decay, stream()), c.id)
    e.assert_bands(c.id)
    compare('ema-' + c.id, mode, e.v, b.ref, b.S, 4)


def build_sq(c, mode):
    """One fmaf: correctly rounded; the allowance of one ulp covers the double rounding of the fp64 reference (k = 0)."""
    g = fill(key('sq', c.id, 'g'), (c.n,), mode, 1000)
    acc = fill(key('sq', c.id, 'acc'), (c.n,), mode, 1 << 22).abs()
    ref = R.sq_accumulate(acc, g)
    assert mode == 'bound' or (float(ref.max()) < 2 ** 24 and is_f32(ref))
    return case(g=g, acc=acc, ref=ref)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(FLAT)
@steady
def test_sq_accumulate_forms(c, mode):
    from rick_amd._lib import lib
    b = build_sq(c, mode)
    acc, g = Guarded(c.n, b.acc, off=1), fenced(b.g, off=1)
    ok(lib.rick_sq_accumulate_f32(p(acc), p(g), c.n, stream()), c.id)
    acc.assert_bands(c.id)
    compare('sq-' + c.id, mode, acc.v, b.ref, b.ref, 0)


# --------------------------------------------------------------------------------------------- rick_filter_reduce_f32
FILTER = [case(id=f'outer{o}-F{f}-inner{i}', outer=o, nf=f, inner=i) for o in (1, 3) for f in (1, 3, 4, 5, 9) for i in (1, 63, 64, 65, 144, 200)]


def build_filter(c, mode):
    """inner * outer terms per filter, then the wave's 6 shuffle levels and the product with scale: inner * outer + 7 roundings.
    filter_stride > inner and outer_stride > nfilters * filter_stride, NaN in every gap."""
    X = fill(key('filter', c.id), (c.outer, c.nf, c.inner), mode, 7)
    fs = c.inner + 3
    os_ = c.nf * fs + 5
    flat = torch.full((c.outer * os_,), float('nan'))
    for o in range(c.outer):
        for f in range(c.nf):
            flat[o * os_ + f * fs:o * os_ + f * fs + c.inner] = X[o, f]
    scale = 2.0 ** -3
    ref, S = R.filter_reduce(X, scale)
    assert mode == 'bound' or (is_f32(ref) and float(S.max()) / scale < 2 ** 24)
    assert int(torch.isnan(flat).sum()) == flat.numel() - X.numel() and (c.nf == 1 or float(ref.min()) < float(ref.max()))
    return case(flat=flat, fs=fs, os=os_, scale=scale, ref=ref, S=S)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(FILTER)
@steady
def test_filter_reduce_forms(c, mode):
    from rick_amd._lib import lib
    b = build_filter(c, mode)
    x, out = fenced(b.flat), Guarded(c.nf)
    ok(lib.rick_filter_reduce_f32(p(x), p(out), c.outer, b.os, c.nf, b.fs, c.inner, b.scale, stream()), c.id)
    out.assert_bands(c.id)
    compare('filter-' + c.id, mode, out.v, b.ref, b.S, c.inner * c.outer + 7)


# --------------------------------------------------------------------------------------------------- minibatch stddev
MBSTD = [case(id=f'B{B}-groups{g}-P{P}-C{C}', B=B, groups=g, P=P, C=C) for B, g, P, C in
         ((3, 3, 1, 3), (4, 2, 3, 341), (3, 1, 5, 205), (4, 1, 13, 160), (4, 1, 300, 4), (6, 3, 5, 416), (2, 2, 3, 341))]


def build_mbstd(c):
    x = synth_tensor(key('mbstd', c.id, 'x'), (c.B, c.P, c.C))
    gout = synth_tensor(key('mbstd', c.id, 'g'), (c.B, c.P, c.C + 1))
    stat, gx = R.mbstd_compose(x, gout, c.groups, torch.float64)
    stat32, gx32 = R.mbstd_compose(x, gout, c.groups, torch.float32)
    return case(x=x, gout=gout, stat=stat, gx=gx, stat32=stat32, gx32=gx32, stat_bound=R.mbstd_stat_bound(x, c.groups))


def run_mbstd(x, gout, B, P, C, groups, what):
    from rick_amd._lib import lib
    xd, gd = fenced(x), fenced(gout)
    out, stat, gx = Guarded(B * P * (C + 1)), Guarded(groups), Guarded(B * P * C)
    ok(lib.rick_mbstd_fwd_f32(p(xd), p(out), p(stat), B, P, C, groups, stream()), what)
    ok(lib.rick_mbstd_bwd_f32(p(xd), p(gd), p(gx), B, P, C, groups, stream()), what)
    for b in (out, stat, gx):
        b.assert_bands(what)
    return out.v.cpu().reshape(B, P, C + 1), stat.v.cpu(), gx.v.cpu().reshape(B, P, C)


@gpu
@params(MBSTD)
@steady
def test_mbstd_forms(c):
    b = build_mbstd(c)
    gs = c.B // c.groups
    out, stat, gx = run_mbstd(b.x, b.gout, c.B, c.P, c.C, c.groups, c.id)
    assert torch.equal(out[..., :c.C], b.x), 'out[..., :C] is not x'
    for g in range(c.groups):
        run = out[g * gs:(g + 1) * gs, :, c.C]
        assert bool((run.reshape(-1).view(torch.int32) == stat[g:g + 1].view(torch.int32)).all()), f'channel C of run {g} is not stat[{g}]'
    if gs > 1:
        assert len(set(stat.tolist())) == c.groups, 'two runs with the same statistic'
    within('mbstd-' + c.id, stat, b.stat, b.stat_bound, 'stat')
    print(f'mbstd-{c.id} stat: device {float((stat.double() - b.stat).abs().max()):.3e}  fp32 composition {float((b.stat32.double() - b.stat).abs().max()):.3e}  '
          f'derived bound {float(b.stat_bound.max()):.3e}')
    if gs == 1:
        assert torch.equal(gx, b.gout[..., :c.C]), 'gs = 1: gx is not gout[..., :C]'
    err, base = float((gx.double() - b.gx).abs().max()), float((b.gx32.double() - b.gx).abs().max())
    print(f'mbstd-{c.id} gx: device {err:.3e}  fp32 composition {base:.3e}  bound {4 * base:.3e}')
    assert err <= 4 * base, f'gx: {err:.3e} > 4 x {base:.3e}'
    if c.groups > 1:                # include/rick_hip.h: a grouped call is the separate calls, unchanged
        for g in range(c.groups):
            sl = slice(g * gs, (g + 1) * gs)
            o1, s1, g1 = run_mbstd(b.x[sl], b.gout[sl], gs, c.P, c.C, 1, f'{c.id} run {g} alone')
            same_bits(out[sl], o1, f'run {g}: out')
            same_bits(stat[g:g + 1], s1, f'run {g}: stat')
            same_bits(gx[sl], g1, f'run {g}: gx')


# ------------------------------------------------------------------------------------------------------- image batch
IMAGES = [case(id='B1-5x7', N=3, H=5, W=7, index=[2], flip=[1]), case(id='B5-5x7', N=3, H=5, W=7, index=[2, 2, 1, 0, 0], flip=[1, 0, 1, 1, 0]),
          case(id='B65-512x512-cap', N=2, H=512, W=512, index=[1 - (b * 5 % 3) % 2 for b in range(65)], flip=[(b * 3 % 5) % 2 for b in range(65)])]


def build_images(c):
    """N source images with distinct content and a decoy behind them that no case samples (constant 77)."""
    gen = torch.Generator().manual_seed(c.H * 1000 + c.W)
    src = torch.randint(0, 256, (c.N + 1, c.H, c.W, 3), generator=gen).to(torch.uint8)
    src[c.N] = 77
    assert all(not torch.equal(src[i], src[j]) for i in range(c.N) for j in range(i)) and max(c.index) < c.N and len(c.index) == len(c.flip)
    assert len(c.index) == 1 or (set(c.flip) == {0, 1} and len(set(c.index)) < len(c.index) and any(a > b for a, b in zip(c.index, c.index[1:])))
    return src


@gpu
@params(IMAGES)
@steady
def test_image_batch_forms(c):
    from rick_amd._lib import lib
    src, B, table = build_images(c), len(c.index), R.image_table()
    assert table[0] == -1.0 and table[255] == 1.0 and len(set(table.tolist())) == 256
    images, index = FencedInts(src, 0xFF), FencedInts(torch.tensor(c.index, dtype=torch.int64), c.N)
    flip, out = FencedInts(torch.tensor(c.flip, dtype=torch.uint8), 0xFF), Guarded(B * 3 * c.H * c.W)
    ok(lib.rick_image_batch_f32(images.v.data_ptr(), index.v.data_ptr(), flip.v.data_ptr(), p(out), c.N, c.H, c.W, B, stream()), c.id)
    out.assert_bands(c.id)
    got, tab, imgs = out.v.view(B, 3, c.H, c.W), torch.from_numpy(table).to(DEV), images.v.view(c.N + 1, c.H, c.W, 3)
    if B <= 5:
        assert np.array_equal(got.cpu().numpy().view(np.uint32), R.image_batch(src.numpy(), c.index, c.flip, table).view(np.uint32))
        return
    seen = torch.zeros(256, dtype=torch.bool, device=DEV)
    for b in range(B):              # image by image on the device: the table lookup is pure indexing
        im = imgs[c.index[b]]
        im = im.flip(1) if c.flip[b] else im
        assert torch.equal(got[b].view(torch.int32), tab[im.long()].permute(2, 0, 1).contiguous().view(torch.int32)), f'image {b} of the batch'
        seen[im.reshape(-1).long()] = True
    assert bool(seen.all())


# ---------------------------------------------------------------------------------------------------- host-only tests
def test_case_tables_reach_every_form_and_stay_exact():
    """No device: the launchers' choices, replayed, reach every form the tables are there for; the exponent rule's clamps; every
    builder's own assertions (exact cases are fp32 numbers, inputs are non-degenerate)."""
    # ew_grid: one pass / a second pass for some threads only
    assert [trips(n, ew_blocks(n)) for n in N_LIST] == [(0, 1), (0, 1), (0, 1), (0, 1), (1, 2)] and {c.n for c in ADAM} == set(N_LIST) == {c.n for c in FLAT}
    assert [ew_blocks(n) for n in N_LIST] == [1, 1, 2, 391, EW_BLOCKS] and {c.mask for c in ADAM} == {0, 1}
    assert trips(BIG, ew_blocks(BIG)) == (1, 2) and [c.rows * c.C // 4 for c in ASS] == [1, 257, BIG, 9, 272] and {c.C for c in ASS} == {4, 36, 64}
    # split_pack / split_unpack: blocks of 256 threads, eight passes each
    n4s = [s.npix * s.C // 4 for s in PACK_SHAPES]
    assert n4s == [1, 255, 256, 257, 6149, 9, 261, 6147] and [split_blocks(n) for n in n4s] == [1, 1, 1, 1, 4, 1, 1, 4]
    assert [trips(n, split_blocks(n)) for n in n4s] == [(0, 1), (0, 1), (1, 1), (1, 2), (6, 7), (0, 1), (1, 2), (6, 7)]
    assert {h.clamp for h in PACK_HEADERS} == {None, 'zero', 'low', 'high'} and {h.a1 is None for h in PACK_HEADERS} == {True, False}
    assert any(math.frexp(h.coef)[0] != 0.5 for h in PACK_HEADERS) and all(h.a0[1] != 0 for h in PACK_HEADERS)
    # the exponent rule in integers: T + 1 = 14 is the smallest biased exponent it places, 253 the largest
    for bound, scale, clamp in ((1.0, 2.0 ** 13, None), (2.0 ** -113, 2.0 ** 126, None), (2.0 ** -114, 2.0 ** 126, 'low'), (1e-45, 2.0 ** 126, 'low'),
                                (2.0 ** 126 * 1.5, 2.0 ** -113, None), (2.0 ** 127, 2.0 ** -113, 'high'), (0.0, 1.0, 'zero'), (float(f32(1e4)), 1.0, None)):
        s, u, cl = R.pow2_scale(bound)
        assert (float(s), cl) == (scale, clamp) and float(s) * float(u) == 1.0, (bound, float(s), cl)
    for s, h in PACK_RUNS:
        build_pack(s, h)
    # amax_kernel: one block / two blocks / four blocks with a later pass; every tail length; both signs planted
    assert [amax_blocks(n) for n in AMAX_N] == [1, 1, 1, 1, 1, 1, 1, 1, 2, 4] and {n % 4 for n in AMAX_N} == {0, 1, 2, 3}
    assert amax_positions(7) == [0, 2, 4, 5, 6] and amax_positions(3) == [0, 1, 2] and amax_positions(4) == [0, 2]
    assert amax_positions(8192) == [0, 4609, 8190] and amax_positions(3 * 8192 + 5)[1] == (1024 + 2560) * 4 + 1 and len(amax_positions(1023)) == 5
    blk, nb = amax_block_of(3 * 8192 + 5)
    assert nb == 4 and blk[-1] == 0 and blk[4 * 1024] == 0 and blk[4 * 1023] == 3 and blk[(1024 + 2560) * 4 + 1] == 2
    assert all(len(amax_positions(n)) > 1 or n == 1 for n in AMAX_N)
    # bound tail: the eight presence combinations, each noise operand alone, every size on both operands
    assert {(c.noise == 'nw+noise', c.bias, c.mul) for c in BOUND_TAIL} == {(n, b, m) for n in (False, True) for b in (0, 1) for m in (0, 1)}
    assert {'nw', 'noise'} <= {c.noise for c in BOUND_TAIL} and {c.nbias for c in BOUND_TAIL} == set(BT_SIZES) == {c.nmul for c in BOUND_TAIL}
    assert len({c.id for c in BOUND_TAIL}) == len(BOUND_TAIL)
    for c in BOUND_TAIL:
        build_bound_tail(c)
    # Adam, EMA, Fisher: every exact case (the large ones included: they are cheap on the host)
    for c in ADAM:
        mask, (p0, m0, v0) = adam_mask(c), adam_state(c, 'exact')
        adam_expect(ADAM_EXACT, p0, adam_grad(c, 'exact', 1), m0, v0, mask, 'exact')
    assert ADAM_EXACT.beta1 != 0 and ADAM_REAL.bc[0][0] == 1.0 and abs(ADAM_REAL.beta2 - 0.99 ** 0.8) < 1e-7 and {c.count for c in PREPARE} == {1, 255, 256, 257, 600}
    for mode in MODES:
        for c in FLAT:
            build_ema(c, mode)
            build_sq(c, mode)
        for c in ASS:
            if c.rows < BIG:
                build_ass(c, mode)
        for c in FILTER:
            build_filter(c, mode)
    # filter_reduce: blocks of four waves, idle waves in the last one; lanes with no / one / several elements
    assert {f: filter_idle_waves(f) for f in (1, 3, 4, 5, 9)} == {1: 3, 3: 1, 4: 0, 5: 3, 9: 3} and {c.outer for c in FILTER} == {1, 3}
    assert {c.inner for c in FILTER} == {1, 63, 64, 65, 144, 200} and len(FILTER) == 60
    # minibatch stddev: P * C below / just below / just above / twice the block; the copy and G loops with and without a stride
    forms = {c.id: mbstd_forms(c.B, c.groups, c.P, c.C) for c in MBSTD}
    assert {c.P * c.C for c in MBSTD} == {3, 1023, 1025, 2080, 1200} and {f[0] for f in forms.values()} == {(0, 1), (1, 2), (2, 3)}
    assert {c.B // c.groups for c in MBSTD} == {1, 2, 3, 4} and {c.groups for c in MBSTD} == {1, 2, 3} and {(c.C + 1) % 2 for c in MBSTD} == {0, 1}
    assert forms['B4-groups1-P300-C4'][2] == (1, 2) and all(f[2] == (0, 1) for k, f in forms.items() if 'P300' not in k)
    assert all(math.isqrt(c.P) ** 2 != c.P or c.P == 1 for c in MBSTD)
    for c in MBSTD:
        b = build_mbstd(c)
        assert bool((b.stat_bound > 0).all()) and bool(((b.stat32.double() - b.stat).abs() <= b.stat_bound).all()), 'the fp32 composition misses the derived bound'
    # image batch: the 65 535-block cap is reached by the last case only
    assert [image_blocks(len(c.index), c.H, c.W) for c in IMAGES] == [1, 1, 65535] and 65 * 512 * 512 > 65535 * 256
    for c in IMAGES[:2]:
        build_images(c)
    assert IMAGES[0].W % 2 == 1 and IMAGES[0].H != IMAGES[0].W and set(IMAGES[2].index) == {0, 1} and set(IMAGES[2].flip) == {0, 1}


# --------------------------------------------------------------------------------------------- GPU: argument tables
def refuse(fn, good, bads, guards, what, rc_want=EINVAL):
    """Every (label, overrides) of `bads` applied to the valid argument list `good` returns rc_want (RICK_EINVAL, or 0 for the
    zero-size calls); nothing is launched, so every guarded buffer is untouched."""
    seen = set()
    for label, over in bads:
        assert label not in seen and set(over) <= set(good), label
        seen.add(label)
        args = dict(good)
        args.update(over)
        rc = fn(*args.values())
        assert rc == rc_want, f'{what}: {label}: rc = {rc}'
    torch.cuda.synchronize()
    for gd in guards:
        assert gd.untouched(), f'{what}: {"refused" if rc_want else "zero-size"}, and something was written'


def nulls(*names):
    return [('null ' + n, {n: None}) for n in names]


def nonpos(*names):
    return [(f'{n} = 0', {n: 0}) for n in names] + [(f'{n} = -1', {n: -1}) for n in names]


def off4(gd):
    return gd.v.data_ptr() + 4


@gpu
@steady
def test_split_entry_points_refuse_on_the_host():
    from rick_amd._lib import lib
    st = stream()
    a, b, w0, w1, out, out2, hdr = (Guarded(4096) for _ in range(7))
    outs = [out, out2, hdr]
    good = dict(x=p(a), out=p(out), hdr=p(hdr), a0=p(w0), a1=p(w1), coef=1.0, npix=8, C=8, st=st)
    refuse(lib.rick_split_pack_f32, good, nulls('x', 'out', 'hdr', 'a0') + [('npix = -1', {'npix': -1})] + nonpos('C') + [('C & 3', {'C': 6}), ('coef = 0', {'coef': 0.0}),
           ('coef < 0', {'coef': -1.0}), ('coef NaN', {'coef': float('nan')}), ('x 4 bytes off', {'x': off4(a)}), ('out 4 bytes off', {'out': off4(out)}),
           ('hdr 4 bytes off', {'hdr': off4(hdr)})], outs, 'rick_split_pack_f32')
    refuse(lib.rick_split_pack_f32, good, [('npix = 0', {'npix': 0})], outs, 'rick_split_pack_f32', 0)
    good = dict(pk=p(a), hdr=p(b), out=p(out), npix=8, C=8, st=st)
    refuse(lib.rick_split_unpack_f32, good, nulls('pk', 'hdr', 'out') + [('npix = -1', {'npix': -1})] + nonpos('C') + [('C & 3', {'C': 6}), ('pk 4 bytes off', {'pk': off4(a)}),
           ('out 4 bytes off', {'out': off4(out)}), ('hdr 4 bytes off', {'hdr': off4(b)})], outs, 'rick_split_unpack_f32')
    refuse(lib.rick_split_unpack_f32, good, [('npix = 0', {'npix': 0})], outs, 'rick_split_unpack_f32', 0)
    good = dict(a=p(a), b=p(b), y=p(out), ys=p(out2), hdr=p(hdr), wa=p(w0), wb=p(w1), rows=8, C=8, alpha=0.5, st=st)
    refuse(lib.rick_add_scale_split_f32, good, nulls('a', 'b', 'y', 'ys', 'hdr', 'wa', 'wb') + [('rows = -1', {'rows': -1})] + nonpos('C') + [('C & 3', {'C': 6}),
           ('alpha = 0', {'alpha': 0.0})] + [(f'{n} 4 bytes off', {n: off4(g)}) for n, g in (('a', a), ('b', b), ('y', out), ('ys', out2), ('hdr', hdr))],
           outs, 'rick_add_scale_split_f32')
    refuse(lib.rick_add_scale_split_f32, good, [('rows = 0', {'rows': 0})], outs, 'rick_add_scale_split_f32', 0)
    good = dict(x=p(a), n=64, word=p(out), st=st)
    refuse(lib.rick_amax_f32, good, nulls('x', 'word') + [('n = -1', {'n': -1}), ('x 4 bytes off', {'x': off4(a)})], outs, 'rick_amax_f32')
    refuse(lib.rick_amax_f32, good, [('n = 0', {'n': 0})], outs, 'rick_amax_f32', 0)
    good = dict(out=p(out), w0=p(w0), c0=1.0, nw=p(a), noise=p(w1), bias=p(b), nbias=8, gain=1.0, mul=p(b), nmul=8, st=st)
    refuse(lib.rick_bound_tail_f32, good, nulls('out', 'w0') + [('c0 = 0', {'c0': 0.0}), ('c0 < 0', {'c0': -1.0}), ('gain = 0', {'gain': 0.0}), ('gain < 0', {'gain': -2.0}),
           ('nbias = -1', {'nbias': -1}), ('nmul = -1', {'nmul': -1})], outs, 'rick_bound_tail_f32')


@gpu
@steady
def test_state_entry_points_refuse_on_the_host():
    from rick_amd._lib import lib
    st = stream()
    pp, g, m, v, bc, x = (Guarded(4096) for _ in range(6))
    mask = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    steps = torch.full((64,), 5, dtype=torch.int32, device=DEV)
    outs = [pp, g, m, v, bc]
    good = dict(p=p(pp), g=p(g), m=p(m), v=p(v), mask=mask.data_ptr(), n=64, lr=0.1, b1=0.5, b2=0.75, eps=1e-8, bc1=0.5, bc2=0.25, st=st)
    refuse(lib.rick_masked_adam_f32, good, nulls('p', 'g', 'm', 'v') + [('n = -1', {'n': -1})], outs, 'rick_masked_adam_f32')
    refuse(lib.rick_masked_adam_f32, good, [('n = 0', {'n': 0})], outs, 'rick_masked_adam_f32', 0)
    good = dict(p=p(pp), g=p(g), m=p(m), v=p(v), mask=mask.data_ptr(), n=64, lr=0.1, b1=0.5, b2=0.75, eps=1e-8, bc=p(x), st=st)
    refuse(lib.rick_masked_adam_dev_f32, good, nulls('p', 'g', 'm', 'v', 'bc') + [('n = -1', {'n': -1})], outs, 'rick_masked_adam_dev_f32')
    refuse(lib.rick_masked_adam_dev_f32, good, [('n = 0', {'n': 0})], outs, 'rick_masked_adam_dev_f32', 0)
    good = dict(steps=steps.data_ptr(), first=1, count=3, b1=0.5, b2=0.75, bc=p(bc), st=st)
    refuse(lib.rick_adam_prepare_f32, good, nulls('steps', 'bc') + [('first = -1', {'first': -1}), ('count = 0', {'count': 0}), ('count = -1', {'count': -1})], outs, 'rick_adam_prepare_f32')
    assert bool((steps == 5).all())
    good = dict(ema=p(pp), p=p(x), n=64, decay=0.5, st=st)
    refuse(lib.rick_ema_f32, good, nulls('ema', 'p') + [('n = -1', {'n': -1})], outs, 'rick_ema_f32')
    refuse(lib.rick_ema_f32, good, [('n = 0', {'n': 0})], outs, 'rick_ema_f32', 0)
    good = dict(acc=p(pp), g=p(x), n=64, st=st)
    refuse(lib.rick_sq_accumulate_f32, good, nulls('acc', 'g') + [('n = -1', {'n': -1})], outs, 'rick_sq_accumulate_f32')
    refuse(lib.rick_sq_accumulate_f32, good, [('n = 0', {'n': 0})], outs, 'rick_sq_accumulate_f32', 0)
    good = dict(x=p(x), out=p(pp), outer=2, os=64, nf=3, fs=16, inner=8, scale=1.0, st=st)
    refuse(lib.rick_filter_reduce_f32, good, nulls('x', 'out') + nonpos('outer', 'nf', 'inner'), outs, 'rick_filter_reduce_f32')
    good = dict(x=p(x), out=p(pp), stat=p(g), B=4, P=3, C=5, groups=2, st=st)
    refuse(lib.rick_mbstd_fwd_f32, good, nulls('x', 'out', 'stat') + nonpos('B', 'P', 'C', 'groups') + [('B % groups', {'groups': 3})], outs, 'rick_mbstd_fwd_f32')
    good = dict(x=p(x), gout=p(m), gx=p(pp), B=4, P=3, C=5, groups=2, st=st)
    refuse(lib.rick_mbstd_bwd_f32, good, nulls('x', 'gout', 'gx') + nonpos('B', 'P', 'C', 'groups') + [('B % groups', {'groups': 3})], outs, 'rick_mbstd_bwd_f32')
    good = dict(images=mask.data_ptr(), index=steps.data_ptr(), flip=mask.data_ptr(), out=p(pp), N=1, H=4, W=4, B=2, st=st)
    refuse(lib.rick_image_batch_f32, good, nulls('images', 'index', 'flip', 'out') + nonpos('N', 'H', 'W', 'B'), outs, 'rick_image_batch_f32')
