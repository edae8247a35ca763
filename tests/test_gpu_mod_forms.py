"""Every dispatch form of the style path (rick_amd/csrc/modulation.hip: wsq, demod, demod_bwd_s, demod_bwd_w, their four
*_multi bank kernels, modbank_fwd, modbank_bwd, equal_linear) and of the short-batch linear family (rick_amd/csrc/linear.hip:
linear_fwd / linear_finish with split-K over a workspace, linear_dgrad with split-O over a workspace, linear_wgrad), through the
C ABI, against the fp64 expressions of tests/mod_f64.py.  The method is that of tests/test_gpu_thin_forms.py;
tests/forms_common.py holds what the forms files share.

Two checks, neither with a measured tolerance; every case runs both:

  exact   operands are small non-zero sign-mixed integers; scale, alpha, bias_mul, slope and gain are powers of two; the
          demodulation coefficients d fed to the backward kernels are powers of two and gd integers, so t = -0.5 d^3 gd and all
          that follows is exact.  sum |terms| < 2**24 units for every output element (asserted on the CPU before the launch), so
          every partial sum in any order is an fp32 number and the device result must be torch.equal to the fp64 result cast to
          fp32.  This is the check that pins indexing, tails, offsets and the two-stage sums.
  bound   standard-normal operands (rick_amd.synth), scale = alpha = 1 / sqrt(K), slope 0.2, gain sqrt(2); per output element
          |dev - ref64| <= (n + k) * 2**-24 * sum |terms| + one ulp of the result: n summed terms, k further roundings of the
          kernel's written association (counted next to each builder).

Three places hold a transcendental and get a derived bound (compare_demod, build_equal_linear):
  demod, exact   the sum is an exact integer, tot + eps rounds once (half an ulp of the argument: a quarter of an ulp of d),
                 rsqrtf is documented at 1 ulp: |dev - ref64| <= 2 ulp of the fp64 result cast to fp32.  Every case runs with
                 eps = 1e-8 and with eps = 3: a dropped eps moves the result by far more.
  demod, bound   all terms are positive: the relative error of the sum is at most (I + 2) * 2**-24 (the square of s, the I-term
                 sum, the + eps); d inherits half of it, plus the 2 ulp above.
  equal_linear with pixelnorm (bound mode only)   see build_equal_linear.

Around every launch: outputs, workspaces and flat buffers lie between sentinel bands that stay intact; workspaces have exactly
rick_linear_{fwd,dgrad}_workspace_floats floats; every read-only operand is a view with NaN on both sides (the layers of a flat
bank buffer have NaN between them); elements a form must not write keep the sentinel (the gaps of the flat outputs, the padding
between gb and the next gW of the modulation bank's gradient layout, the slices of a frozen layer).  Inputs are asserted
non-degenerate (distinct weight rows, both signs, non-constant outputs).  The bank kernels are held bit-equal to the per-layer
kernels in both modes, as include/rick_hip.h promises.

Every rejection written in the entry points returns RICK_EINVAL with nothing launched and nothing written (the two tests at the
end), the LDS limits among them: B * K * 4 bytes > 64 KB for rick_modbank_fwd_f32, > 160 KB for rick_equal_linear_f32 — the
discriminator's first final layer sends [4, 8192] (128 KB) through that entry in every no-grad pass, so shapes between 64 KB and
160 KB are cases here (EL_LARGE), not refusals.

The case builders and the launcher replays are host-only (test_case_tables_reach_every_form_and_stay_exact).

What these cases caught when one line of a scratch copy of the sources was changed (each mutant run once on an MI355X):
  demod_bwd_s_kernel   clamp o1 = ... : O - 1               all 72 of test_demod_bwd_s_forms (the wave that reaches O drops its
                                                            last row at every O: O3-I8-B1-exact reads 36 where -6 is due)
  demod_kernel         i + 192 <= I                         test_demod_forms[I200-*], all 27 (lane 8 reads past its row: with
                                                            O = 1 that is the NaN fence); the other 108 stay green
  demod_multi_kernel   eps dropped                          test_demod_bank_forms[B1|B3|B8-exact-eps3] (1806 x the 2-ulp bound);
                                                            eps = 1e-8 cannot see it and stays green
  linear_finish_kernel bias[i]                              test_linear_fwd_forms[K1028|K2304-*-B5-bias-*], all 12 (rows b > 0
                                                            read past the bias into the NaN fence); B = 1 and the unsplit K stay green
  linear_dgrad_kernel  r + 4 < rows, remainder loop kept    all 26 of test_linear_dgrad_forms green: the same terms in another order
  modbank_bwd_kernel   bias branch c0 + r <= ds.C           test_modbank_bwd_forms[*-acc0-*], all 24 (a zero lands in the padding
                                                            after gb / in the guard band); accumulate = 1 adds that zero and stays green
"""
import math
import types

import numpy as np
import pytest
import torch

from rick_amd.synth import synth_tensor
from tests import mod_f64 as R
from tests.forms_common import DEV, SENT, Fenced, Guarded, cdiv, f32, fenced, ints, p, scales, stream

gpu = pytest.mark.gpu
U = 2.0 ** -24
MODES = ('exact', 'bound')
EINVAL = 22
GAP = 4                       # floats between the layers of a flat bank buffer (NaN in operands, the sentinel in outputs)
MOD_MAXB, MB_MAXB, EL_MAXB, LN_MAXB = 32, 8, 16, 16
DBS_WAVES, WSQ_KMAX, MB_ROWS, LN_KSLICE = 16, 9, 32, 1024
PN_EPS = 1e-8


def case(**kw):
    return types.SimpleNamespace(**kw)


def params(cases):
    return pytest.mark.parametrize('c', cases, ids=[c.id for c in cases])


# ------------------------------------------------------------------------------------------ host-side launcher replay
def demod_lane_steps(I):
    """demod_kernel / demod_multi_kernel: {(unrolled steps, remainder steps)} over the 64 lanes of a wave."""
    steps = set()
    for lane in range(64):
        i, unrolled, rem = lane, 0, 0
        while i + 192 < I:
            i, unrolled = i + 256, unrolled + 1
        while i < I:
            i, rem = i + 64, rem + 1
        steps.add((unrolled, rem))
    return steps


def dbs_wave_forms(O):
    """demod_bwd_s_kernel's split of the o range over its 16 waves: the set of what a wave does."""
    o_per = cdiv(O, DBS_WAVES)
    forms = set()
    for wave in range(DBS_WAVES):
        o0 = wave * o_per
        o1 = o0 + o_per if o0 + o_per < O else O
        if o0 > O:
            forms.add('o0>O')
        if o0 >= o1:
            forms.add('empty')
            continue
        rows = o1 - o0
        forms.add(('unroll' if rows // 4 else '') + ('+rem' if rows % 4 else ''))
    return forms


def ln_dgrad_rows(K, O):
    slices = max(256 // cdiv(K, 1024), 1)
    return min(max(cdiv(O, slices), 32), 256)


def ln_dgrad_slices(K, O):
    """-> (R, [rows of every row slice])"""
    rows = ln_dgrad_rows(K, O)
    return rows, [min(rows, O - o0) for o0 in range(0, O, rows)]


def ln_fwd_slices(K):
    return [min(LN_KSLICE, K - k0) for k0 in range(0, K, LN_KSLICE)]


def fwd_ws_floats(B, K, O):
    S = len(ln_fwd_slices(K))
    return S * B * O if S > 1 else 0


def dgrad_ws_floats(B, K, O):
    S = len(ln_dgrad_slices(K, O)[1])
    return S * B * K if S > 1 else 0


def block_ranges(counts):
    out, pos = [], 0
    for n in counts:
        out.append(pos)
        pos += n
    return out, pos


def layout(sizes):
    """Float offsets of the layers of a flat buffer, GAP floats apart, every start 16-byte aligned -> (offsets, total)."""
    offs, pos = [], 0
    for n in sizes:
        offs.append(pos)
        pos += cdiv(n, 4) * 4 + GAP
    return offs, pos


def modbank_grad_layout(C, K):
    """ModulationBank's gradient layout: [W_0 | b_0 | W_1 | b_1 ...], every start 16-byte aligned."""
    gw_off, gb_off, pos = [], [], 0
    for c in C:
        gw_off.append(pos)
        pos += c * K
        gb_off.append(pos)
        pos += (c + 3) // 4 * 4
    return gw_off, gb_off, pos


# ------------------------------------------------------------------------------------------------------------ inputs
def fill(key, shape, mode, amp):
    """exact: non-zero integers in [-amp, amp], both signs; bound: standard normal."""
    return synth_tensor('modforms/' + key, shape) if mode == 'bound' else ints(key, shape, amp)


def positive(key, shape, mode, amp):
    return synth_tensor('modforms/' + key, shape).abs() + 0.05 if mode == 'bound' else ints(key, shape, amp).abs()


def weight(key, shape, mode, amp):
    """fill(), drawn again under another key until no two rows are equal and no row is constant (4-column rows of small integers
    do collide)."""
    for t in range(16):
        W = fill(f'{key}#{t}' if t else key, shape, mode, amp)
        rows = W.reshape(-1, shape[-1])
        if torch.unique(rows, dim=0).shape[0] == rows.shape[0] and bool((rows.min(1).values < rows.max(1).values).all()):
            return W
    raise AssertionError('no draw with distinct rows')


def pow2(mode, e, K):
    """scale / alpha: 2**e (exact) or 1 / sqrt(K) as fp32 (bound)."""
    return 2.0 ** e if mode == 'exact' else f32(1 / math.sqrt(K))


def act_consts(mode):
    return (0.25, 2.0) if mode == 'exact' else (f32(0.2), f32(math.sqrt(2)))


def self_check(mode, ref, S, unit=1.0, rows=None, signed=None):
    """The premises of both checks, asserted about the inputs before the device is touched; `signed`: operands (bias and old values
    among them) that must be non-zero everywhere and, from 32 elements on, of both signs."""
    if mode == 'exact':
        assert float(S.max()) / unit < 2 ** 24, f'sum |terms| = {float(S.max())} in units of {unit}: not exact in fp32'
        assert torch.equal(ref.float().double(), ref), 'the fp64 result is not an fp32 number'
    if ref.numel() > 1:
        assert float(ref.min()) < float(ref.max()), 'constant output: the case cannot tell operands apart'
    if rows is not None and rows.shape[-1] >= 4 and rows.numel() // rows.shape[-1] > 1:
        flat = rows.reshape(-1, rows.shape[-1])
        assert torch.unique(flat, dim=0).shape[0] == flat.shape[0], 'two equal weight rows'
    for t in signed or ():
        assert t.numel() < 32 or (bool((t > 0).any()) and bool((t < 0).any())), 'an operand of one sign'
        assert bool((t != 0).all()), 'a zero operand'


# ------------------------------------------------------------------------------------------------------ case builders
def build_wsq(c, mode):
    """K products and sums; scale * scale on the host and the final product are two further roundings: k = 2."""
    w = fill(c.id + '/w', (c.O, c.I, c.K), mode, 7)
    scale = pow2(mode, -1, c.K)
    ref, S = R.wsq(w, scale)
    self_check(mode, ref, S, scale * scale, signed=[w])
    return case(w=w, scale=scale, ref=ref, S=S, n=c.K, k=2)


def build_demod(c, mode, eps):
    s = fill(c.id + '/s', (c.B, c.I), mode, 3)
    wsq = positive(c.id + '/wsq', (c.O, c.I), mode, 7)
    eps = f32(eps)
    ref, tot = R.demod(s, wsq, eps)
    if mode == 'exact':
        assert float(tot.max()) + eps < 2 ** 24 and torch.equal(tot, tot.round())
    assert c.B * c.O == 1 or float(ref.min()) < float(ref.max())
    assert bool((s > 0).any()) and bool((s < 0).any()) and bool((wsq > 0).all())
    return case(s=s, wsq=wsq, eps=eps, ref=ref)


def build_bwd_s(c, mode):
    """t = ((-0.5 d) d) d gd: three roundings on every term; the O-term sum (wave partials, then the fixed-order combine); the
    final 2 s * tot: one more.  k = 4."""
    s = fill(c.id + '/s', (c.B, c.I), mode, 3)
    wsq = fill(c.id + '/wsq', (c.O, c.I), mode, 7)
    d = scales(c.id + '/d', (c.B, c.O), mode)
    gd = fill(c.id + '/gd', (c.B, c.O), mode, 3)
    ref, S = R.demod_bwd_s(s, wsq, d, gd)
    self_check(mode, ref, S, 2.0 ** -4, signed=[s, wsq, gd])
    return case(s=s, wsq=wsq, d=d, gd=gd, ref=ref, S=S, n=c.O, k=4)


def build_bwd_w(c, mode):
    """B terms t * s^2 (three roundings in t, one in s^2), then scale * scale on the host, (2 scale2) * acc and w * f: k = 7;
    accumulate adds one term."""
    w = fill(c.id + '/w', (c.O, c.I, c.K), mode, 7)
    s = fill(c.id + '/s', (c.B, c.I), mode, 3)
    d = scales(c.id + '/d', (c.B, c.O), mode)
    gd = fill(c.id + '/gd', (c.B, c.O), mode, 3)
    old = fill(c.id + '/old', (c.O, c.I, c.K), mode, 50) if c.acc else None
    scale = pow2(mode, -1, c.K)
    ref, S = R.demod_bwd_w(w, s, d, gd, scale, old)
    self_check(mode, ref, S, 2.0 ** -5, signed=[w, s, gd] + ([old] if c.acc else []))
    return case(w=w, s=s, d=d, gd=gd, old=old, scale=scale, ref=ref, S=S, n=c.B + int(c.acc), k=7)


def build_modbank(c, mode):
    """Forward: K products and the bias, n = K + 1; the product with scale: k = 1.
    Backward: B terms (+ the old value), the product with scale: k = 1 (gW), k = 0 (gb)."""
    L = len(c.C)
    lat = fill(c.id + '/lat', (c.B, c.n_latent, c.K), mode, 3)
    scale = pow2(mode, -4, c.K)
    W = [weight(f'{c.id}/W{l}', (c.C[l], c.K), mode, 7) for l in range(L)]
    b = [fill(f'{c.id}/b{l}', (c.C[l],), mode, 9) if c.has_b[l] else None for l in range(L)]
    gs = [fill(f'{c.id}/gs{l}', (c.B, c.C[l]), mode, 7) for l in range(L)]
    out = case(lat=lat, scale=scale, W=W, b=b, gs=gs, fwd=[], bwd=[], old_w=[], old_b=[])
    for l in range(L):
        ll = lat[:, c.lat_idx[l]]
        ref, S = R.modbank_fwd(ll, W[l], b[l], scale)
        self_check(mode, ref, S, scale, rows=W[l], signed=[W[l]] + ([b[l]] if c.has_b[l] else []))
        out.fwd.append((ref, S))
        old_w = fill(f'{c.id}/oldw{l}', (c.C[l], c.K), mode, 50) if c.acc else None
        old_b = fill(f'{c.id}/oldb{l}', (c.C[l],), mode, 50) if c.acc else None
        gw, gb = R.modbank_bwd(ll, gs[l], scale, old_w, old_b)
        self_check(mode, gw[0], gw[1], scale, signed=[gs[l]] + ([old_w, old_b] if c.acc else []))
        self_check(mode, gb[0], gb[1])
        out.bwd.append((gw, gb))
        out.old_w.append(old_w)
        out.old_b.append(old_b)
    return out


def build_equal_linear(c, mode):
    """K products and the bias: n = K + 1; the products with scale, bias_mul, slope and gain: k = 4.

    pixelnorm (bound mode only): q = sum_k x^2 has positive terms, so its relative error is at most K * 2**-24; q / K (fp32
    division is correctly rounded) and + 1e-8 round once each: (K + 2) * 2**-24 on the argument.  rsqrtf halves that and adds
    its own 1 ulp (2 * 2**-24 relative); x * rn rounds once more: every x' carries a relative error of at most
    e = ((K + 2) / 2 + 3) * 2**-24, which every term of the dot product inherits: the bound is (n + k) * 2**-24 * S + e * S."""
    x = fill(c.id + '/x', (c.B, c.K), mode, 3)
    W = weight(c.id + '/W', (c.O, c.K), mode, 7)
    bias = fill(c.id + '/bias', (c.O,), mode, 9) if c.bias else None
    scale = pow2(mode, -4, c.K)
    bias_mul = 0.5 if mode == 'exact' else f32(0.01)
    slope, gain = act_consts(mode)
    assert not (c.pn and mode == 'exact')
    ref, S = R.equal_linear(x, W, bias, scale, bias_mul, c.act, slope, gain, f32(PN_EPS) if c.pn else None)
    self_check(mode, ref, S, scale * slope, rows=W, signed=[W, x] + ([bias] if c.bias else []))
    extra = ((c.K + 2) / 2 + 3) if c.pn else 0
    return case(x=x, W=W, bias=bias, scale=scale, bias_mul=bias_mul, slope=slope, gain=gain, ref=ref, S=S, n=c.K + 1, k=4 + extra)


def build_linear_fwd(c, mode):
    """K products and the bias: n = K + 1 (the slices' partial sums are part of that sum); alpha and bias_mul: k = 2."""
    x = fill(c.id + '/x', (c.B, c.K), mode, 3)
    W = weight(c.id + '/W', (c.O, c.K), mode, 7)
    bias = fill(c.id + '/bias', (c.O,), mode, 9) if c.bias else None
    alpha = pow2(mode, -4, c.K)
    bias_mul = 0.5 if mode == 'exact' else f32(0.01)
    ref, S = R.linear_fwd(x, W, bias, alpha, bias_mul)
    self_check(mode, ref, S, alpha, rows=W, signed=[W, x] + ([bias] if c.bias else []))
    return case(x=x, W=W, bias=bias, alpha=alpha, bias_mul=bias_mul, ref=ref, S=S, n=c.K + 1, k=2)


def build_linear_dgrad(c, mode):
    """O terms; alpha: k = 1."""
    g = fill(c.id + '/g', (c.B, c.O), mode, 3)
    W = weight(c.id + '/W', (c.O, c.K), mode, 7)
    alpha = pow2(mode, -4, c.K)
    ref, S = R.linear_dgrad(g, W, alpha)
    self_check(mode, ref, S, alpha, signed=[W, g])
    return case(g=g, W=W, alpha=alpha, ref=ref, S=S, n=c.O, k=1)


def build_linear_wgrad(c, mode):
    """B terms (+ the old value); alpha or bias_mul: k = 1."""
    g = fill(c.id + '/g', (c.B, c.O), mode, 3)
    x = weight(c.id + '/x', (c.B, c.K), mode, 7)
    alpha = pow2(mode, -4, c.K)
    bias_mul = 0.5 if mode == 'exact' else f32(0.01)
    old_w = fill(c.id + '/oldw', (c.O, c.K), mode, 50) if c.acc else None
    old_b = fill(c.id + '/oldb', (c.O,), mode, 50) if c.acc else None
    gw, gb = R.linear_wgrad(g, x, alpha, bias_mul, old_w, old_b)
    self_check(mode, gw[0], gw[1], alpha, signed=[g, x] + ([old_w, old_b] if c.acc else []))
    self_check(mode, gb[0], gb[1], bias_mul)
    plain = R.linear_wgrad(g, x, alpha, bias_mul)
    return case(g=g, x=x, alpha=alpha, bias_mul=bias_mul, old_w=old_w, old_b=old_b, gw=gw, gb=gb, plain=plain, n=c.B + int(c.acc), k=1)


# ------------------------------------------------------------------------------------------------------- case tables
WSQ_SHAPES = ((1, 5), (16, 16), (12, 25))                    # O * I = 5, 256, 300
WSQ = [case(id=f'K{K}-O{O}-I{I}', O=O, I=I, K=K) for K in (1, 9, 16) for O, I in WSQ_SHAPES]
# three layers of different K each; together every (K, O * I) of the per-layer table; a ragged last block before another layer
WSQ_BANKS = [case(id='K1.9.16', layers=[(1, 5, 1), (12, 25, 9), (16, 16, 16)]), case(id='K9.16.1', layers=[(12, 25, 16), (1, 5, 9), (16, 16, 1)]),
             case(id='K16.1.9', layers=[(16, 16, 9), (12, 25, 1), (1, 5, 16)])]

DEMOD = [case(id=f'I{I}-O{O}-B{B}', I=I, O=O, B=B) for I in (8, 64, 200, 256, 320) for O in (1, 6, 8) for B in (1, 5, 32)]
DEMOD_EPS = (1e-8, 3.0)
DEMOD_BANKS = [case(id=f'B{B}', B=B, layers=[(6, 200), (1, 8), (8, 320), (6, 64), (8, 256), (1, 320)]) for B in (1, 3, 8)]

BWD_S = [case(id=f'O{O}-I{I}-B{B}', O=O, I=I, B=B) for O in (3, 17, 70, 128) for I in (8, 64, 100) for B in (1, 5, 32)]
BWD_S_BANKS = [case(id=f'B{B}', B=B, layers=[(3, 8), (128, 100), (17, 64), (70, 100), (128, 8), (3, 64)]) for B in (1, 8)]

BWD_W = [case(id=f'K{K}-O{O}-I{I}-B{B}-acc{acc}', O=O, I=I, K=K, B=B, acc=acc)
         for K in (1, 9) for O, I in ((1, 5), (12, 25), (3, 100)) for B in (1, 5) for acc in (0, 1)]
# (O, I, K, live): the middle layer of the first table has gw = NULL
BWD_W_BANKS = [case(id=f'{name}-B{B}', B=B, layers=layers) for B in (1, 8) for name, layers in
               (('frozen-mid', [(12, 25, 9, True), (3, 100, 1, False), (1, 5, 9, True)]), ('live', [(3, 100, 1, True), (12, 25, 9, True), (1, 5, 1, True)]))]


def _modbank_cases():
    out = []
    for K in (256, 512):
        for B in (1, 3, 8):
            for acc in (0, 1):
                # C: a layer smaller than a wave's 8 rows / one full block / C % 32 != 0 / three blocks, the last ragged.  The frozen
                # layer lies between live ones; its gs is NaN.  role: which gradients the backward launch produces.
                out.append(case(id=f'K{K}-B{B}-main-acc{acc}', K=K, B=B, acc=acc, n_latent=3, C=[3, 32, 40, 70, 40], lat_idx=[2, 0, 2, 1, 0],
                                has_b=[True, True, False, True, True], role=['wb', 'w', '', 'wb', 'b']))
                out.append(case(id=f'K{K}-B{B}-single-acc{acc}', K=K, B=B, acc=acc, n_latent=3, C=[70], lat_idx=[1], has_b=[True], role=['wb']))
    return out


MODBANK = _modbank_cases()
MODBANK_FWD = [c for c in MODBANK if not c.acc]

EL_FLAGS = [(bias, act, pn) for bias in (0, 1) for act in (0, 1) for pn in (0, 1)]


def _el(B, K, O, bias, act, pn):
    return case(id=f'B{B}-K{K}-O{O}{"-bias" if bias else ""}{"-act" if act else ""}{"-pn" if pn else ""}', B=B, K=K, O=O, bias=bias, act=act, pn=pn)


EQUAL_LINEAR = [_el(B, K, O, *f) for B in (1, 5, 16) for K in (4, 260, 512) for O in (1, 7, 9, 40) for f in EL_FLAGS]
# more than the 64 KB of LDS a kernel gets by default: just above it / the discriminator's first final layer in a no-grad pass of
# four images (128 KB: EqualLinear.forward sends it here) / exactly the 160 KB the entry point accepts
EL_LARGE = [_el(16, 1028, 9, 1, 1, 0), _el(4, 8192, 9, 1, 1, 0), _el(4, 8192, 7, 0, 0, 1), _el(16, 2560, 9, 1, 1, 1), _el(16, 2560, 7, 1, 0, 0)]
EQUAL_LINEAR += EL_LARGE
EQUAL_LINEAR_RUNS = [(c, m) for c in EQUAL_LINEAR for m in MODES if not (c.pn and m == 'exact')]

LINEAR_FWD = [case(id=f'K{K}-O{O}-B{B}{"-bias" if bias else ""}', K=K, O=O, B=B, bias=bias)
              for K in (4, 260, 1024, 1028, 2304) for O in (1, 7, 9) for B in (1, 5, 16) for bias in (0, 1)]
LINEAR_DGRAD = [case(id=f'K{K}-O{O}-B{B}', K=K, O=O, B=B) for K, O in ((4, 1), (260, 33), (1028, 70), (1024, 32)) for B in (1, 5, 16)]
LINEAR_DGRAD.append(case(id='K16384-O544-B2', K=16384, O=544, B=2))          # ln_dgrad_rows returns R = 34 > 32: a 36 MB weight
LINEAR_WGRAD = [case(id=f'K{K}-O{O}-B{B}-{which}-acc{acc}', K=K, O=O, B=B, which=which, acc=acc)
                for K in (4, 1028) for O in (1, 9) for B in (1, 5, 16) for which in ('gw', 'gb', 'both') for acc in (0, 1)]


# ---------------------------------------------------------------------------------------------------- host-only tests
def test_case_tables_reach_every_form_and_stay_exact():
    """No device: the launchers' choices, replayed, reach every form the tables are there for; the replays agree with the
    library's own host functions; every exact case satisfies sum |terms| < 2**24 units (asserted inside the builders)."""
    from rick_amd._lib import lib
    # demod_kernel / demod_multi_kernel: idle lanes / no unroll / lanes on both sides of the unroll / full unroll / unroll + remainder
    assert demod_lane_steps(8) == {(0, 1), (0, 0)} and demod_lane_steps(64) == {(0, 1)}
    assert demod_lane_steps(200) == {(1, 0), (0, 3)} and demod_lane_steps(256) == {(1, 0)} and demod_lane_steps(320) == {(1, 1)}
    assert {c.I for c in DEMOD} == {8, 64, 200, 256, 320} == {I for c in DEMOD_BANKS for _, I in c.layers}
    assert {c.O for c in DEMOD} == {1, 6, 8} == {O for c in DEMOD_BANKS for O, _ in c.layers}      # O % 4 != 0: waves return early
    assert {c.B for c in DEMOD} == {1, 5, MOD_MAXB} and {c.B for c in DEMOD_BANKS} == {1, 3, MB_MAXB}
    assert all(len({I for _, I in c.layers}) > 1 for c in DEMOD_BANKS)
    # demod_bwd_s_kernel
    assert dbs_wave_forms(3) == {'+rem', 'empty', 'o0>O'} and dbs_wave_forms(17) == {'+rem', 'empty', 'o0>O'}
    assert dbs_wave_forms(70) == {'unroll+rem', 'empty', 'o0>O'} and dbs_wave_forms(128) == {'unroll'}
    assert cdiv(17, DBS_WAVES) == 2 and 9 * 2 > 17                                                     # wave 8: one row; wave 9: o0 = 18 > O
    assert {c.O for c in BWD_S} == {3, 17, 70, 128} == {O for c in BWD_S_BANKS for O, _ in c.layers}
    assert {c.I for c in BWD_S} == {8, 64, 100} == {I for c in BWD_S_BANKS for _, I in c.layers}
    assert {c.B for c in BWD_S} == {1, 5, MOD_MAXB} and {c.B for c in BWD_S_BANKS} == {1, MB_MAXB}
    # wsq: K > WSQ_KMAX takes the bank's direct path; the last block of a layer has npair < 256
    assert {c.K for c in WSQ} == {1, 9, 16} and max(c.K for c in WSQ) > WSQ_KMAX
    assert {c.O * c.I for c in WSQ} == {5, 256, 300}
    for c in WSQ_BANKS:
        assert len({K for _, _, K in c.layers}) == 3
    assert {(O * I, K) for c in WSQ_BANKS for O, I, K in c.layers} == {(c.O * c.I, c.K) for c in WSQ}
    for O, I in WSQ_SHAPES:
        assert lib.rick_demod_blocks_wsq(O, I) == cdiv(O * I, 256)
    for O in (1, 6, 8):
        assert lib.rick_demod_blocks(O) == cdiv(O, 4)
    for I in (8, 64, 100):
        assert lib.rick_demod_blocks_bwd_s(I) == cdiv(I, 64)
    assert all((c.O * c.I) % 256 for c in BWD_W) and {c.K for c in BWD_W} == {1, 9} and {c.acc for c in BWD_W} == {0, 1}
    assert any([live for *_, live in c.layers] == [True, False, True] for c in BWD_W_BANKS)
    # modulation bank
    for c in MODBANK:
        blk, total = block_ranges([cdiv(C, MB_ROWS) for C in c.C])
        assert [lib.rick_modbank_blocks(C) for C in c.C] == [cdiv(C, MB_ROWS) for C in c.C] and total == sum(cdiv(C, MB_ROWS) for C in c.C)
        assert c.K % 256 == 0 and c.B <= MB_MAXB and max(c.lat_idx) < c.n_latent == 3
    main = next(c for c in MODBANK if 'main' in c.id)
    assert {3, 32, 40, 70} <= set(main.C) and min(main.C) < 8 and main.lat_idx != sorted(main.lat_idx) and not all(main.has_b)
    assert set(main.role) == {'wb', 'w', 'b', ''} and main.role.index('') not in (0, len(main.role) - 1)
    assert {c.K for c in MODBANK} == {256, 512} and {c.B for c in MODBANK} == {1, 3, 8} and any(len(c.C) == 1 for c in MODBANK)
    gw_off, gb_off, total = modbank_grad_layout(main.C, 256)
    assert all(o % 4 == 0 for o in gw_off) and any(gb_off[l] + main.C[l] < gw_off[l + 1] for l in range(len(main.C) - 1))     # padding exists
    # equal_linear
    assert {(c.B, c.K, c.O) for c in EQUAL_LINEAR if c not in EL_LARGE} == {(B, K, O) for B in (1, 5, 16) for K in (4, 260, 512) for O in (1, 7, 9, 40)}
    assert {(c.bias, c.act, c.pn) for c in EQUAL_LINEAR} == set(EL_FLAGS)
    for name, vals in (('B', (1, 5, 16)), ('K', (4, 260, 512)), ('O', (1, 7, 9, 40))):
        for v in vals:
            for flag in ('bias', 'act', 'pn'):
                assert {getattr(c, flag) for c in EQUAL_LINEAR if getattr(c, name) == v} == {0, 1}, (name, v, flag)
    assert [c.B * c.K * 4 for c in EL_LARGE] == [65792, 128 * 1024, 128 * 1024, 160 * 1024, 160 * 1024] and 16 * 2564 * 4 > 160 * 1024
    assert all(c.B * c.K * 4 <= 64 * 1024 for c in EQUAL_LINEAR if c not in EL_LARGE) and 8 * 2304 * 4 > 64 * 1024
    # linear forward: S = 1 / a split with a 4-column last slice / a split with a 256-column last slice
    assert [ln_fwd_slices(K) for K in (4, 260, 1024, 1028, 2304)] == [[4], [260], [1024], [1024, 4], [1024, 1024, 256]]
    for c in LINEAR_FWD:
        assert lib.rick_linear_fwd_workspace_floats(c.B, c.K, c.O) == fwd_ws_floats(c.B, c.K, c.O)
    assert {(c.K, c.bias) for c in LINEAR_FWD} == {(K, b) for K in (4, 260, 1024, 1028, 2304) for b in (0, 1)}
    # linear data gradient
    assert ln_dgrad_slices(4, 1) == (32, [1]) and ln_dgrad_slices(260, 33) == (32, [32, 1]) and ln_dgrad_slices(1028, 70) == (32, [32, 32, 6])
    assert ln_dgrad_slices(1024, 32) == (32, [32]) and ln_dgrad_slices(16384, 544) == (34, [34] * 16)
    assert ln_dgrad_rows(16384 - 1024, 544) == 32 and ln_dgrad_rows(16384, 512) == 32                  # one k block or 32 rows fewer: R = 32
    assert {ln_dgrad_rows(c.K, c.O) for c in LINEAR_DGRAD} == {32, 34}
    for c in LINEAR_DGRAD:
        assert lib.rick_linear_dgrad_workspace_floats(c.B, c.K, c.O) == dgrad_ws_floats(c.B, c.K, c.O)
    assert {(c.which, c.acc) for c in LINEAR_WGRAD} == {(w, a) for w in ('gw', 'gb', 'both') for a in (0, 1)}
    assert {c.O % 8 for c in LINEAR_WGRAD} == {1}                                                       # the last block has one row
    # every exact case
    for c in WSQ:
        build_wsq(c, 'exact')
    for c in DEMOD:
        for eps in DEMOD_EPS:
            build_demod(c, 'exact', eps)
    for c in BWD_S:
        build_bwd_s(c, 'exact')
    for c in BWD_W:
        build_bwd_w(c, 'exact')
    for bank, builder in ((WSQ_BANKS, wsq_layers), (BWD_S_BANKS, bwd_s_layers), (BWD_W_BANKS, bwd_w_layers)):
        for c in bank:
            builder(c, 'exact')
    for c in DEMOD_BANKS:
        for eps in DEMOD_EPS:
            demod_layers(c, 'exact', eps)
    for c in MODBANK:
        build_modbank(c, 'exact')
    for c, mode in EQUAL_LINEAR_RUNS:
        if mode == 'exact':
            build_equal_linear(c, mode)
    for c in LINEAR_FWD:
        build_linear_fwd(c, 'exact')
    for c in LINEAR_DGRAD:
        if c.K * c.O > 1 << 21:                 # the 36 MB weight is built on the device run only: 544 terms of at most 3 * 7
            assert c.O * 3 * 7 < 2 ** 24
            continue
        build_linear_dgrad(c, 'exact')
    for c in LINEAR_WGRAD:
        build_linear_wgrad(c, 'exact')


# ----------------------------------------------------------------------------------------------------- device helpers
def ulp32(ref):
    """One ulp of ref cast to fp32, per element (fp64)."""
    _, e = torch.frexp(ref.float())
    return 2.0 ** (e.double() - 24)


def compare(cid, mode, got, ref, S, n, k, what='out'):
    got = got.detach().cpu().reshape(ref.shape)
    if mode == 'exact':
        exp = ref.float()
        bad = got != exp
        assert not bool(bad.any()), (f'{cid} {what}: {int(bad.sum())} of {bad.numel()} elements differ, first at '
                                     f'{tuple(bad.nonzero()[0].tolist())}: {float(got[bad][0])} != {float(exp[bad][0])}')
    else:
        err = (got.double() - ref).abs()
        bound = (n + k) * U * S + 2.0 ** -23 * ref.abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f'{cid} {what}: max |err| / bound = {worst:.3f} (n = {n}, k = {k})')
        assert bool((err <= bound).all()), f'{cid} {what}: |err| up to {worst:.3f} x the a-priori bound'


def compare_demod(cid, mode, got, ref, I):
    """exact: 2 ulp of the fp64 result cast to fp32; bound: + half of (I + 2) * 2**-24 relative (see the module's docstring)."""
    got = got.detach().cpu().reshape(ref.shape)
    err = (got.double() - ref).abs()
    bound = 2 * ulp32(ref) + (0.5 * (I + 2) * U * ref.abs() if mode == 'bound' else 0.0)
    worst = float((err / bound).max())
    print(f'{cid}: max |err| / bound = {worst:.3f}')
    assert bool((err <= bound).all()), f'{cid}: |err| up to {worst:.3f} x the derived bound ({mode})'


def same(a, b, what):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'{what}: {int((a != b).sum())} of {a.numel()} elements differ'


def table(arr):
    return torch.from_numpy(arr.view(np.uint8).copy()).to(DEV)


def fenced_flat(offs, total, tensors):
    """The layers of a flat operand at their offsets, NaN between and around them (None: the layer's slice stays NaN)."""
    fd = Fenced(total)
    for o, t in zip(offs, tensors):
        if t is not None:
            fd.v[o:o + t.numel()].copy_(t.reshape(-1))
    return fd


def rest_is_sentinel(gd, offs, sizes, what):
    """Everything of a guarded flat output outside the layers' slices still holds the sentinel."""
    gd.assert_bands(what)
    keep = torch.ones(gd.v.numel(), dtype=torch.bool, device=DEV)
    for o, n in zip(offs, sizes):
        keep[o:o + n] = False
    assert bool((gd.v[keep] == SENT).all()), f'{what}: wrote between the layers'


def ok(rc, what):
    assert rc == 0, f'{what}: rc = {rc}'
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------- per-layer launches (device)
def run_wsq(b, O, I, K, what):
    from rick_amd._lib import lib
    w, out = fenced(b.w), Guarded(O * I)
    ok(lib.rick_wsq_f32(p(w), p(out), O, I, K, b.scale, stream()), what)
    out.assert_bands(what)
    return out.v.cpu()


def run_demod(b, B, I, O, what):
    from rick_amd._lib import lib
    s, wsq, out = fenced(b.s), fenced(b.wsq), Guarded(B * O)
    ok(lib.rick_demod_f32(p(s), p(wsq), p(out), B, I, O, b.eps, stream()), what)
    out.assert_bands(what)
    return out.v.cpu()


def run_bwd_s(b, B, I, O, what):
    from rick_amd._lib import lib
    s, wsq, d, gd, out = fenced(b.s), fenced(b.wsq), fenced(b.d), fenced(b.gd), Guarded(B * I)
    ok(lib.rick_demod_bwd_s_f32(p(s), p(wsq), p(d), p(gd), p(out), B, I, O, stream()), what)
    out.assert_bands(what)
    return out.v.cpu()


def run_bwd_w(b, B, I, O, K, acc, what, old=None):
    from rick_amd._lib import lib
    w, s, d, gd = fenced(b.w), fenced(b.s), fenced(b.d), fenced(b.gd)
    out = Guarded(O * I * K, old if acc else None)
    ok(lib.rick_demod_bwd_w_f32(p(w), p(s), p(d), p(gd), p(out), B, I, O, K, b.scale, acc, stream()), what)
    out.assert_bands(what)
    return out.v.cpu()


# ------------------------------------------------------------------------------------------------ demodulation banks
def wsq_layers(c, mode):
    return [build_wsq(case(id=f'wsqbank-{c.id}/L{l}', O=O, I=I, K=K), mode) for l, (O, I, K) in enumerate(c.layers)]


def demod_layers(c, mode, eps):
    return [build_demod(case(id=f'demodbank-{c.id}/L{l}', O=O, I=I, B=c.B), mode, eps) for l, (O, I) in enumerate(c.layers)]


def bwd_s_layers(c, mode):
    return [build_bwd_s(case(id=f'bwdsbank-{c.id}/L{l}', O=O, I=I, B=c.B), mode) for l, (O, I) in enumerate(c.layers)]


def bwd_w_layers(c, mode):
    return [build_bwd_w(case(id=f'bwdwbank-{c.id}/L{l}', O=O, I=I, K=K, B=c.B, acc=1), mode) for l, (O, I, K, _) in enumerate(c.layers)]


def demod_table(O, I, K, B, w=None, wsq=None, gw=None, scale2=None):
    """rick_demod_desc rows for layers of [O, I, K]; pointers from lists of device buffers (or None) -> (array, layout)."""
    from rick_amd.op.modconv import _DM_DESC
    L = len(O)
    s_off, s_total = layout([B * i for i in I])
    d_off, d_total = layout([B * o for o in O])
    blk_wsq, n_wsq = block_ranges([cdiv(o * i, 256) for o, i in zip(O, I)])
    blk_demod, n_demod = block_ranges([cdiv(o, 4) for o in O])
    blk_bwd_s, n_bwd_s = block_ranges([cdiv(i, 64) for i in I])
    arr = np.zeros(L, dtype=_DM_DESC)
    for l in range(L):
        arr[l] = (p(w[l]) or 0 if w else 0, p(wsq[l]) or 0 if wsq else 0, p(gw[l]) or 0 if gw else 0, s_off[l], d_off[l], O[l], I[l],
                  K[l], scale2[l] if scale2 else 0.0, blk_wsq[l], blk_demod[l], blk_bwd_s[l], 0)
    return arr, case(s_off=s_off, s_total=s_total, d_off=d_off, d_total=d_total, n_wsq=n_wsq, n_demod=n_demod, n_bwd_s=n_bwd_s)


# ------------------------------------------------------------------------------------------------- GPU: demodulation
@gpu
@pytest.mark.parametrize('mode', MODES)
@params(WSQ)
def test_wsq_forms(c, mode):
    b = build_wsq(c, mode)
    compare('wsq-' + c.id, mode, run_wsq(b, c.O, c.I, c.K, c.id), b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(WSQ_BANKS)
def test_wsq_bank_forms(c, mode):
    from rick_amd._lib import lib
    bs = wsq_layers(c, mode)
    O, I, K = zip(*c.layers)
    w = [fenced(b.w) for b in bs]
    out = [Guarded(o * i) for o, i in zip(O, I)]
    scale2 = [np.float32(b.scale) * np.float32(b.scale) for b in bs]
    arr, lay = demod_table(O, I, K, 1, w=w, wsq=out, scale2=scale2)
    assert [lib.rick_demod_blocks_wsq(o, i) for o, i in zip(O, I)] == [cdiv(o * i, 256) for o, i in zip(O, I)]
    tab = table(arr)
    ok(lib.rick_wsq_multi_f32(tab.data_ptr(), len(O), lay.n_wsq, stream()), c.id)
    for l, b in enumerate(bs):
        out[l].assert_bands(f'{c.id} layer {l}')
        compare(f'wsqbank-{c.id} layer {l}', mode, out[l].v, b.ref, b.S, b.n, b.k)
        same(out[l].v, run_wsq(b, O[l], I[l], K[l], c.id), f'{c.id} layer {l}: bank against rick_wsq_f32')


DEMOD_RUNS = [(c, 'exact', eps) for c in DEMOD for eps in DEMOD_EPS] + [(c, 'bound', 1e-8) for c in DEMOD]
DEMOD_BANK_RUNS = [(c, 'exact', eps) for c in DEMOD_BANKS for eps in DEMOD_EPS] + [(c, 'bound', 1e-8) for c in DEMOD_BANKS]


def _eps_id(c, mode, eps):
    return f'{c.id}-{mode}-eps{"3" if eps == 3.0 else "1e-8"}'


@gpu
@pytest.mark.parametrize('c,mode,eps', DEMOD_RUNS, ids=[_eps_id(*r) for r in DEMOD_RUNS])
def test_demod_forms(c, mode, eps):
    b = build_demod(c, mode, eps)
    compare_demod('demod-' + _eps_id(c, mode, eps), mode, run_demod(b, c.B, c.I, c.O, c.id), b.ref, c.I)


@gpu
@pytest.mark.parametrize('c,mode,eps', DEMOD_BANK_RUNS, ids=[_eps_id(*r) for r in DEMOD_BANK_RUNS])
def test_demod_bank_forms(c, mode, eps):
    from rick_amd._lib import lib
    bs = demod_layers(c, mode, eps)
    O, I = zip(*c.layers)
    wsq = [fenced(b.wsq) for b in bs]
    arr, lay = demod_table(O, I, [1] * len(O), c.B, wsq=wsq)
    s_flat = fenced_flat(lay.s_off, lay.s_total, [b.s for b in bs])
    d_flat = Guarded(lay.d_total)
    tab = table(arr)
    assert [lib.rick_demod_blocks(o) for o in O] == [cdiv(o, 4) for o in O]
    ok(lib.rick_demod_multi_f32(p(s_flat), p(d_flat), tab.data_ptr(), len(O), lay.n_demod, c.B, max(I), bs[0].eps, stream()), c.id)
    rest_is_sentinel(d_flat, lay.d_off, [c.B * o for o in O], c.id)
    for l, b in enumerate(bs):
        got = d_flat.v[lay.d_off[l]:lay.d_off[l] + c.B * O[l]]
        compare_demod(f'demodbank-{_eps_id(c, mode, eps)} layer {l}', mode, got, b.ref, I[l])
        same(got, run_demod(b, c.B, I[l], O[l], c.id), f'{c.id} layer {l}: bank against rick_demod_f32')


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(BWD_S)
def test_demod_bwd_s_forms(c, mode):
    b = build_bwd_s(c, mode)
    compare('bwds-' + c.id, mode, run_bwd_s(b, c.B, c.I, c.O, c.id), b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(BWD_S_BANKS)
def test_demod_bwd_s_bank_forms(c, mode):
    from rick_amd._lib import lib
    bs = bwd_s_layers(c, mode)
    O, I = zip(*c.layers)
    wsq = [fenced(b.wsq) for b in bs]
    arr, lay = demod_table(O, I, [1] * len(O), c.B, wsq=wsq)
    s_flat = fenced_flat(lay.s_off, lay.s_total, [b.s for b in bs])
    d_flat = fenced_flat(lay.d_off, lay.d_total, [b.d for b in bs])
    gd_flat = fenced_flat(lay.d_off, lay.d_total, [b.gd for b in bs])
    gs_flat = Guarded(lay.s_total)
    tab = table(arr)
    assert [lib.rick_demod_blocks_bwd_s(i) for i in I] == [cdiv(i, 64) for i in I]
    ok(lib.rick_demod_bwd_s_multi_f32(p(s_flat), p(d_flat), p(gd_flat), p(gs_flat), tab.data_ptr(), len(O), lay.n_bwd_s, c.B, max(O),
                                      stream()), c.id)
    rest_is_sentinel(gs_flat, lay.s_off, [c.B * i for i in I], c.id)
    for l, b in enumerate(bs):
        got = gs_flat.v[lay.s_off[l]:lay.s_off[l] + c.B * I[l]]
        compare(f'bwdsbank-{c.id} layer {l}', mode, got, b.ref, b.S, b.n, b.k)
        same(got, run_bwd_s(b, c.B, I[l], O[l], c.id), f'{c.id} layer {l}: bank against rick_demod_bwd_s_f32')


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(BWD_W)
def test_demod_bwd_w_forms(c, mode):
    b = build_bwd_w(c, mode)
    compare('bwdw-' + c.id, mode, run_bwd_w(b, c.B, c.I, c.O, c.K, c.acc, c.id, b.old), b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(BWD_W_BANKS)
def test_demod_bwd_w_bank_forms(c, mode):
    """The bank always accumulates: it starts from a non-zero gw and equals rick_demod_bwd_w_f32 with accumulate = 1 bit for bit;
    a layer with gw = NULL between two live ones leaves them right and writes nothing."""
    from rick_amd._lib import lib
    bs = bwd_w_layers(c, mode)
    O, I, K, live = zip(*c.layers)
    w = [fenced(b.w) for b in bs]
    gw = [Guarded(o * i * k, b.old) if lv else None for o, i, k, lv, b in zip(O, I, K, live, bs)]
    scale2 = [np.float32(b.scale) * np.float32(b.scale) for b in bs]
    arr, lay = demod_table(O, I, K, c.B, w=w, gw=gw, scale2=scale2)
    assert [int(a['gw'] != 0) for a in arr] == [int(lv) for lv in live]
    s_flat = fenced_flat(lay.s_off, lay.s_total, [b.s for b in bs])
    d_flat = fenced_flat(lay.d_off, lay.d_total, [b.d for b in bs])
    gd_flat = fenced_flat(lay.d_off, lay.d_total, [b.gd if lv else None for b, lv in zip(bs, live)])     # a frozen layer's gd is NaN
    tab = table(arr)
    ok(lib.rick_demod_bwd_w_multi_f32(p(s_flat), p(d_flat), p(gd_flat), tab.data_ptr(), len(O), lay.n_wsq, c.B, stream()), c.id)
    for l, b in enumerate(bs):
        if not live[l]:
            continue
        gw[l].assert_bands(f'{c.id} layer {l}')
        compare(f'bwdwbank-{c.id} layer {l}', mode, gw[l].v, b.ref, b.S, b.n, b.k)
        same(gw[l].v, run_bwd_w(b, c.B, I[l], O[l], K[l], 1, c.id, b.old), f'{c.id} layer {l}: bank against rick_demod_bwd_w_f32, accumulate = 1')


# ------------------------------------------------------------------------------------------------ GPU: modulation bank
def modbank_table(c, W, b, io_off, gw_off, gb_off):
    from rick_amd.op.modconv import _MB_DESC
    blk, total = block_ranges([cdiv(C, MB_ROWS) for C in c.C])
    arr = np.zeros(len(c.C), dtype=_MB_DESC)
    for l in range(len(c.C)):
        arr[l] = (p(W[l]), p(b[l]) or 0, io_off[l], gw_off[l], gb_off[l], c.C[l], c.lat_idx[l], blk[l], 0)
    return arr, total


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(MODBANK_FWD)
def test_modbank_fwd_forms(c, mode):
    from rick_amd._lib import lib
    b = build_modbank(c, mode)
    L = len(c.C)
    lat, W, bias = fenced(b.lat), [fenced(w) for w in b.W], [fenced(v) for v in b.b]
    io_off, io_total = layout([c.B * C for C in c.C])
    arr, total = modbank_table(c, W, bias, io_off, [-1] * L, [-1] * L)
    assert [int(a['b'] != 0) for a in arr] == [int(h) for h in c.has_b]
    out, tab = Guarded(io_total), table(arr)
    ok(lib.rick_modbank_fwd_f32(p(lat), c.B, c.n_latent, c.K, tab.data_ptr(), L, total, b.scale, p(out), stream()), c.id)
    rest_is_sentinel(out, io_off, [c.B * C for C in c.C], c.id)
    for l in range(L):
        ref, S = b.fwd[l]
        compare(f'modbank-fwd-{c.id} layer {l}', mode, out.v[io_off[l]:io_off[l] + c.B * c.C[l]], ref, S, c.K + 1, 1)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(MODBANK)
def test_modbank_bwd_forms(c, mode):
    """The gradient buffer is laid out as ModulationBank lays it out; only the slices the launch must produce are pre-filled
    (accumulate) — everything else, the padding after every gb included, holds the sentinel before and after."""
    from rick_amd._lib import lib
    b = build_modbank(c, mode)
    L = len(c.C)
    lat, W = fenced(b.lat), [fenced(w) for w in b.W]
    io_off, io_total = layout([c.B * C for C in c.C])
    gs = fenced_flat(io_off, io_total, [g if r else None for g, r in zip(b.gs, c.role)])        # a frozen layer's gs is NaN
    gw_all, gb_all, grad_floats = modbank_grad_layout(c.C, c.K)
    gw_off = [o if 'w' in r else -1 for o, r in zip(gw_all, c.role)]
    gb_off = [o if 'b' in r else -1 for o, r in zip(gb_all, c.role)]
    arr, total = modbank_table(c, W, [None] * L, io_off, gw_off, gb_off)
    grad = Guarded(grad_floats)
    offs, sizes = [], []
    for l in range(L):
        for off, n, old in ((gw_off[l], c.C[l] * c.K, b.old_w[l]), (gb_off[l], c.C[l], b.old_b[l])):
            if off >= 0:
                offs.append(off)
                sizes.append(n)
                if c.acc:
                    grad.v[off:off + n].copy_(old.reshape(-1))
    tab = table(arr)
    ok(lib.rick_modbank_bwd_f32(p(lat), p(gs), c.B, c.n_latent, c.K, tab.data_ptr(), L, total, b.scale, p(grad), c.acc, stream()), c.id)
    rest_is_sentinel(grad, offs, sizes, c.id)
    for l in range(L):
        (gw, Sw), (gb, Sb) = b.bwd[l]
        if gw_off[l] >= 0:
            compare(f'modbank-bwd-{c.id} layer {l}', mode, grad.v[gw_off[l]:gw_off[l] + c.C[l] * c.K], gw, Sw, c.B + c.acc, 1, 'gW')
        if gb_off[l] >= 0:
            compare(f'modbank-bwd-{c.id} layer {l}', mode, grad.v[gb_off[l]:gb_off[l] + c.C[l]], gb, Sb, c.B + c.acc, 0, 'gb')


# ------------------------------------------------------------------------------------------------ GPU: equal_linear
@gpu
@pytest.mark.parametrize('c,mode', EQUAL_LINEAR_RUNS, ids=[f'{c.id}-{m}' for c, m in EQUAL_LINEAR_RUNS])
def test_equal_linear_forms(c, mode):
    from rick_amd._lib import lib
    b = build_equal_linear(c, mode)
    x, W, bias, out = fenced(b.x), fenced(b.W), fenced(b.bias), Guarded(c.B * c.O)
    ok(lib.rick_equal_linear_f32(p(x), p(W), p(bias), p(out), c.B, c.K, c.O, b.scale, b.bias_mul, c.act, b.slope, b.gain, c.pn, stream()), c.id)
    out.assert_bands(c.id)
    compare('equal-linear-' + c.id, mode, out.v, b.ref, b.S, b.n, b.k)


# ----------------------------------------------------------------------------------------------------- GPU: linear
def workspace(floats):
    return Guarded(floats) if floats else None


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(LINEAR_FWD)
def test_linear_fwd_forms(c, mode):
    from rick_amd._lib import lib
    b = build_linear_fwd(c, mode)
    x, W, bias, out = fenced(b.x), fenced(b.W), fenced(b.bias), Guarded(c.B * c.O)
    nws = lib.rick_linear_fwd_workspace_floats(c.B, c.K, c.O)
    assert nws == fwd_ws_floats(c.B, c.K, c.O)
    ws = workspace(nws)
    ok(lib.rick_linear_fwd_f32(p(x), p(W), p(bias), p(out), c.B, c.K, c.O, b.alpha, b.bias_mul, p(ws), stream()), c.id)
    out.assert_bands(c.id)
    if ws is not None:
        ws.assert_bands(c.id + ' workspace')
        assert not bool((ws.v == SENT).any()), 'a partial sum was never written'
    compare('linear-fwd-' + c.id, mode, out.v, b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(LINEAR_DGRAD)
def test_linear_dgrad_forms(c, mode):
    from rick_amd._lib import lib
    b = build_linear_dgrad(c, mode)
    g, W, out = fenced(b.g), fenced(b.W), Guarded(c.B * c.K)
    nws = lib.rick_linear_dgrad_workspace_floats(c.B, c.K, c.O)
    assert nws == dgrad_ws_floats(c.B, c.K, c.O)
    ws = workspace(nws)
    ok(lib.rick_linear_dgrad_f32(p(g), p(W), p(out), c.B, c.K, c.O, b.alpha, p(ws), stream()), c.id)
    out.assert_bands(c.id)
    if ws is not None:
        ws.assert_bands(c.id + ' workspace')
        assert not bool((ws.v == SENT).any()), 'a partial sum was never written'
    compare('linear-dgrad-' + c.id, mode, out.v, b.ref, b.S, b.n, b.k)


def run_wgrad(c, b, acc):
    from rick_amd._lib import lib
    g, x = fenced(b.g), fenced(b.x)
    gw = Guarded(c.O * c.K, b.old_w if acc else None) if c.which != 'gb' else None
    gb = Guarded(c.O, b.old_b if acc else None) if c.which != 'gw' else None
    ok(lib.rick_linear_wgrad_f32(p(g), p(x), p(gw), p(gb), c.B, c.K, c.O, b.alpha, b.bias_mul, acc, stream()), c.id)
    for gd in (gw, gb):
        if gd is not None:
            gd.assert_bands(c.id)
    return gw, gb


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(LINEAR_WGRAD)
def test_linear_wgrad_forms(c, mode):
    """accumulate = 1 starts from non-zero old values and is bit-equal to old + the accumulate = 0 result (the kernel rounds the
    product on its own in both modes)."""
    b = build_linear_wgrad(c, mode)
    gw, gb = run_wgrad(c, b, c.acc)
    if gw is not None:
        compare('linear-wgrad-' + c.id, mode, gw.v, b.gw[0], b.gw[1], b.n, b.k, 'gw')
    if gb is not None:
        compare('linear-wgrad-' + c.id, mode, gb.v, b.gb[0], b.gb[1], b.n, b.k, 'gb')
    if c.acc:
        pw, pb = run_wgrad(c, b, 0)
        if gw is not None:
            compare('linear-wgrad-' + c.id, mode, pw.v, b.plain[0][0], b.plain[0][1], c.B, 1, 'gw, accumulate = 0')
            same(gw.v, b.old_w.reshape(-1) + pw.v.cpu(), c.id + ': gw against old + plain')
        if gb is not None:
            same(gb.v, b.old_b + pb.v.cpu(), c.id + ': gb against old + plain')


# --------------------------------------------------------------------------------------------- GPU: argument tables
def refuse(fn, good, bads, guards, what):
    """Every (label, overrides) of `bads` applied to the valid argument list `good` returns RICK_EINVAL; nothing is launched, so
    every guarded buffer is untouched."""
    seen = set()
    for label, over in bads:
        assert label not in seen and set(over) <= set(good), label
        seen.add(label)
        args = dict(good)
        args.update(over)
        rc = fn(*args.values())
        assert rc == EINVAL, f'{what}: {label}: rc = {rc}'
    torch.cuda.synchronize()
    for gd in guards:
        assert gd.untouched(), f'{what}: refused, and something was written'


def nulls(*names):
    return [('null ' + n, {n: None}) for n in names]


def off4(gd):
    return gd.v.data_ptr() + 4


@gpu
def test_modulation_entry_points_refuse_on_the_host():
    from rick_amd._lib import lib
    from rick_amd.op.modconv import _DM_DESC, _MB_DESC
    st = stream()
    a, bb, cc, dd, out = (Guarded(4096) for _ in range(5))
    dm = table(np.zeros(1, dtype=_DM_DESC))
    mb = table(np.zeros(1, dtype=_MB_DESC))
    dims = lambda *names: [(f'{n} = 0', {n: 0}) for n in names] + [(f'{n} = -1', {n: -1}) for n in names]      # noqa: E731
    refuse(lib.rick_wsq_f32, dict(w=p(a), wsq=p(out), O=2, I=4, K=3, scale=1.0, st=st),
           nulls('w', 'wsq') + dims('O', 'I', 'K'), [out], 'rick_wsq_f32')
    refuse(lib.rick_demod_f32, dict(s=p(a), wsq=p(bb), d=p(out), B=2, I=8, O=4, eps=1e-8, st=st),
           nulls('s', 'wsq', 'd') + dims('B', 'I', 'O') + [('B > 32', {'B': MOD_MAXB + 1}), ('LDS: 32 x 513 floats', {'B': 32, 'I': 513})],
           [out], 'rick_demod_f32')
    refuse(lib.rick_demod_bwd_s_f32, dict(s=p(a), wsq=p(bb), d=p(cc), gd=p(dd), gs=p(out), B=2, I=8, O=4, st=st),
           nulls('s', 'wsq', 'd', 'gd', 'gs') + dims('B', 'I', 'O') + [('B > 32', {'B': MOD_MAXB + 1}), ('LDS: 32 x (300 + 1024) floats', {'B': 32, 'O': 300})],
           [out], 'rick_demod_bwd_s_f32')
    assert (32 * 300 + DBS_WAVES * 32 * 64) * 4 > 160 * 1024 >= (32 * 128 + DBS_WAVES * 32 * 64) * 4
    refuse(lib.rick_demod_bwd_w_f32, dict(w=p(a), s=p(bb), d=p(cc), gd=p(dd), gw=p(out), B=2, I=8, O=4, K=3, scale=1.0, acc=0, st=st),
           nulls('w', 's', 'd', 'gd', 'gw') + dims('B', 'I', 'O', 'K'), [out], 'rick_demod_bwd_w_f32')
    refuse(lib.rick_wsq_multi_f32, dict(descs=dm.data_ptr(), n=1, blocks=1, st=st), nulls('descs') + dims('n', 'blocks'), [out], 'rick_wsq_multi_f32')
    refuse(lib.rick_demod_multi_f32, dict(s=p(a), d=p(out), descs=dm.data_ptr(), n=1, blocks=1, B=2, max_I=8, eps=1e-8, st=st),
           nulls('s', 'd', 'descs') + dims('n', 'blocks', 'B', 'max_I') + [('B > 8', {'B': MB_MAXB + 1}), ('LDS: 8 x 2049 floats', {'B': 8, 'max_I': 2049})],
           [out], 'rick_demod_multi_f32')
    refuse(lib.rick_demod_bwd_w_multi_f32, dict(s=p(a), d=p(bb), gd=p(cc), descs=dm.data_ptr(), n=1, blocks=1, B=2, st=st),
           nulls('s', 'd', 'gd', 'descs') + dims('n', 'blocks', 'B') + [('B > 8', {'B': MB_MAXB + 1})], [out], 'rick_demod_bwd_w_multi_f32')
    refuse(lib.rick_demod_bwd_s_multi_f32, dict(s=p(a), d=p(bb), gd=p(cc), gs=p(out), descs=dm.data_ptr(), n=1, blocks=1, B=2, max_O=4, st=st),
           nulls('s', 'd', 'gd', 'gs', 'descs') + dims('n', 'blocks', 'B', 'max_O') + [('B > 8', {'B': MB_MAXB + 1}), ('LDS: 8 x (4100 + 1024) floats', {'B': 8, 'max_O': 4100})],
           [out], 'rick_demod_bwd_s_multi_f32')
    assert (8 * 4100 + DBS_WAVES * 8 * 64) * 4 > 160 * 1024
    refuse(lib.rick_modbank_fwd_f32, dict(lat=p(a), B=2, n_latent=1, K=256, descs=mb.data_ptr(), n=1, blocks=1, scale=1.0, out=p(out), st=st),
           nulls('lat', 'descs', 'out') + dims('B', 'n', 'blocks', 'K') + [('B > 8', {'B': MB_MAXB + 1}), ('K < 256', {'K': 128}), ('K & 255', {'K': 260}), ('K = 384', {'K': 384}),
                                                                          ('LDS: 8 x 2304 floats', {'B': 8, 'K': 2304})],
           [out], 'rick_modbank_fwd_f32')
    refuse(lib.rick_modbank_bwd_f32, dict(lat=p(a), gs=p(bb), B=2, n_latent=1, K=256, descs=mb.data_ptr(), n=1, blocks=1, scale=1.0, grad=p(out), acc=0, st=st),
           nulls('lat', 'gs', 'descs', 'grad') + dims('B', 'n', 'blocks', 'K') + [('B > 8', {'B': MB_MAXB + 1}), ('K < 256', {'K': 128}), ('K & 255', {'K': 260}),
                                                                                  ('grad 4 bytes off', {'grad': off4(out)})],
           [out], 'rick_modbank_bwd_f32')
    refuse(lib.rick_equal_linear_f32, dict(x=p(a), W=p(bb), bias=p(cc), out=p(out), B=2, K=8, O=4, scale=1.0, bias_mul=1.0, act=1, slope=0.25, gain=2.0, pn=1, st=st),
           nulls('x', 'W', 'out') + dims('B', 'K', 'O') + [('B > 16', {'B': EL_MAXB + 1}), ('K < 4', {'K': 2}), ('K & 3', {'K': 6}), ('x 4 bytes off', {'x': off4(a)}),
                                                          ('W 4 bytes off', {'W': off4(bb)}), ('LDS: 16 x 2564 floats', {'B': 16, 'K': 2564})],
           [out], 'rick_equal_linear_f32')


@gpu
def test_linear_entry_points_refuse_on_the_host():
    from rick_amd._lib import lib
    st = stream()
    a, bb, cc, out, out2, ws = (Guarded(4096) for _ in range(6))
    dims = lambda *names: [(f'{n} = 0', {n: 0}) for n in names] + [(f'{n} = -1', {n: -1}) for n in names]      # noqa: E731
    common = dims('B', 'K', 'O') + [('B > 16', {'B': LN_MAXB + 1}), ('K < 4', {'K': 2}), ('K & 3', {'K': 6})]
    assert lib.rick_linear_fwd_workspace_floats(1, 1028, 1) == 2 and lib.rick_linear_dgrad_workspace_floats(1, 260, 33) == 520
    for fn in (lib.rick_linear_fwd_workspace_floats, lib.rick_linear_dgrad_workspace_floats):
        assert fn(0, 8, 4) == fn(2, 2, 4) == fn(2, 8, 0) == -1
    refuse(lib.rick_linear_fwd_f32, dict(x=p(a), W=p(bb), bias=p(cc), out=p(out), B=2, K=8, O=4, alpha=1.0, bias_mul=1.0, ws=p(ws), st=st),
           nulls('x', 'W', 'out') + common + [('x 4 bytes off', {'x': off4(a)}), ('W 4 bytes off', {'W': off4(bb)}),
                                              ('split without a workspace', {'K': 1028, 'O': 1, 'B': 1, 'ws': None})],
           [out, ws], 'rick_linear_fwd_f32')
    refuse(lib.rick_linear_dgrad_f32, dict(g=p(a), W=p(bb), out=p(out), B=2, K=8, O=4, alpha=1.0, ws=p(ws), st=st),
           nulls('g', 'W', 'out') + common + [('W 4 bytes off', {'W': off4(bb)}), ('out 4 bytes off', {'out': off4(out)}), ('workspace 4 bytes off', {'ws': off4(ws)}),
                                              ('split without a workspace', {'K': 8, 'O': 33, 'B': 1, 'ws': None})],
           [out, ws], 'rick_linear_dgrad_f32')
    refuse(lib.rick_linear_wgrad_f32, dict(g=p(a), x=p(bb), gw=p(out), gb=p(out2), B=2, K=8, O=4, alpha=1.0, bias_mul=1.0, acc=0, st=st),
           nulls('g', 'x') + [('neither gw nor gb', {'gw': None, 'gb': None})] + common + [('x 4 bytes off', {'x': off4(bb)}), ('gw 4 bytes off', {'gw': off4(out)})],
           [out, out2], 'rick_linear_wgrad_f32')
