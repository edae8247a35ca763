"""Every dispatch form of the thin products (rick_amd/csrc/thin.hip) and of the NHWC pixel-reduction helpers
(chan_scale / hw_dot* / add_scale in elementwise.hip), through the C ABI, against fp64 expressions written out here.

Two checks, neither with a measured tolerance; every case runs both:

  exact   operands are small integers (wscale, slope, gain, alpha and the divisors powers of two), chosen so that
          max sum |terms| < 2**24 units for every output element (asserted on the CPU before the launch).  Every product
          and every partial sum is then an exactly representable fp32 number in ANY summation order — on the VALU and
          on v_mfma_f32_16x16x4_f32 alike — so the device result must be torch.equal to the fp64 result cast to fp32.
          One dropped, doubled or misplaced term changes an integer.  This is the check that pins indexing, tails and
          the two-stage reductions, at any P.
  bound   standard-normal operands; per output element |dev - ref64| <= (n + k) * 2**-24 * sum |terms| + one ulp of the
          result, n = number of summed terms, k = extra roundings per term of the kernel's documented association
          (counted next to each builder).  The bound holds for any summation order.  It is tight for the channel
          reductions (n <= 2048) — fp16 / bf16 staging or a lost hi/lo half is far outside — and LOOSE for the pixel
          reductions (n up to 65 536: thin_wgrad, hw_dot*); there the exact check carries the weight.

Inputs are not degenerate (distinct weight rows, sign-mixed values, non-zero add / bias / old, non-constant outputs:
asserted), outputs and workspaces sit between sentinel guard bands, and unwritten output elements keep the sentinel.
The case builders and the launcher replay are host-only (test_case_tables_are_exact_and_reach_their_form).
"""
import math
import types
import zlib

import pytest
import torch

from rick_amd.synth import synth_tensor

gpu = pytest.mark.gpu
DEV = 'cuda'
U = 2.0 ** -24
PAD = 64                      # floats of guard band either side (a multiple of 4: the 16-byte alignment is kept)
SENT = -7777.125              # not a multiple of 0.25 .. 1: no exact-mode result can equal it
MODES = ('exact', 'bound')
EINVAL = 22
MFMA_C = (64, 128, 256, 512)
# C -> (lanes per pixel, channel quads per lane) of thin_fwd_kernel<NQ>; every other C % 4 == 0 below 128 is generic
LPP_TABLE = {16: (4, 1), 32: (4, 2), 48: (4, 3), 64: (4, 4), 80: (4, 5), 96: (4, 6), 112: (4, 7), 128: (8, 4), 256: (16, 4),
             512: (32, 4), 1024: (64, 4), 160: (8, 5), 2048: (64, 8)}
GENERIC_LPP = {(4, 1): 1, (4, 3): 4, (8, 1): 2, (8, 2): 2, (8, 3): 4, (8, 4): 4, (36, 3): 8, (40, 3): 8}    # (C, J) -> lanes

# (N, C, P) -> (pixels per block, {(unrolled steps, remainder steps)} over the thread rows of the first and last block) of
# thin_bwdx_cols_kernel; 512 channels at 64 x 64 with a batch of 3 is what the generator launches
BWDX_HANDOFF = {(3, 512, 64 * 64): (12, {(1, 2), (0, 2)}), (3, 512, 4101): (14, {(1, 3), (1, 2)}),
                (3, 128, 128 * 128): (48, {(1, 2), (0, 2)}), (3, 64, 25000): (80, {(1, 1), (0, 3), (0, 2)})}


def case(**kw):
    return types.SimpleNamespace(**kw)


# ------------------------------------------------------------------------------------------ host-side launcher replay
def thin_fwd_form(C, P, J, aligned=True):
    """thin_fwd_launch's choice, replayed: ('mfma', NT, UNR) | ('lpp', lanes, NQ) | ('generic', lanes, 0)."""
    if P % 16 == 0 and C in MFMA_C and aligned:
        return ('mfma', C // 16, 2 if C <= 128 else 1)
    c4 = C // 4
    lpp = 64
    while lpp > 4 and (c4 % lpp or lpp > c4):
        lpp >>= 1
    while lpp > 4 and c4 // lpp < 4 and not c4 % (lpp >> 1):
        lpp >>= 1
    nq = c4 // lpp
    if c4 % lpp or lpp > c4 or nq > 8:
        lpp = 64
        while lpp > c4:
            lpp >>= 1
        if lpp < J:
            lpp = 4
        return ('generic', lpp, 0)
    return ('lpp', lpp, nq)


def thin_bwdx_form(C):
    c4 = C // 4
    return 'cols' if c4 <= 256 and 256 % c4 == 0 else 'fallback'


def thin_bwdx_plan(N, C, P):
    """thin_bwdx_launch's column-owner blocking, replayed: (pixels per block, blocks, steps) with steps the set of
    (unrolled TB_UNR = 4 steps, remainder steps) over every thread row of the first and of the last block."""
    rows = 256 // (C // 4)
    ppb = max(-(-P * N // 1024), 4 * rows)
    ppb = -(-ppb // rows) * rows
    nbx = -(-P // ppb)
    steps = set()
    for npix in {min(ppb, P), P - (nbx - 1) * ppb}:
        for r in range(rows):
            p = r
            unrolled = rem = 0
            while p + 3 * rows < npix:
                p, unrolled = p + 4 * rows, unrolled + 1
            while p < npix:
                p, rem = p + rows, rem + 1
            steps.add((unrolled, rem))
    return ppb, nbx, steps


def thin_wgrad_blocks(P):
    nb = max(1, min(256, -(-P // 64)))
    if -(-P // nb) > 2048:
        nb = -(-P // 2048)
    return nb


def hw_dot_blocks(P):
    return max(1, min(512, -(-P // 16)))


# ------------------------------------------------------------------------------------------------------------ inputs
def fill(key, shape, mode, amp, nonzero=False):
    """exact: integers in [-amp, amp] (as fp32), seeded by the key; bound: standard normal (rick_amd.synth)."""
    if mode == 'bound':
        return synth_tensor('forms/' + key, shape)
    gen = torch.Generator(device='cpu')
    gen.manual_seed(zlib.crc32(key.encode()) & 0x7FFFFFFF)
    t = torch.randint(-amp, amp + 1, tuple(shape), generator=gen).float()
    if nonzero:
        t[t == 0] = float(amp)
    return t


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def self_check(mode, ref, S, unit=1.0, rows=None):
    """The premises of both checks, asserted about the inputs before the device is touched."""
    if mode == 'exact':
        assert float(S.max()) / unit < 2 ** 24, f'sum |terms| = {float(S.max())} units of {unit}: not exact in fp32'
    assert float(ref.min()) < float(ref.max()), 'constant output: the case cannot tell operands apart'
    if rows is not None and rows.shape[-1] >= 4:
        flat = rows.reshape(-1, rows.shape[-1])
        assert torch.unique(flat, dim=0).shape[0] == flat.shape[0], 'two equal weight rows'


def weights(c, key, mode, N, J, C):
    """-> (device operands, Wn fp64 [N, J, C], k, unit).  ToRGB form: W[n,j,c] = (wscale * w[j,c]) * s[n,c] — two extra
    roundings per term (k = 2), formed from the shared [J, C] weight and the style as thin_w does."""
    if c.api == 'torgb':
        w = fill(key + '/w', (J, C), mode, 7)
        s = fill(key + '/s', (N, C), mode, 3, nonzero=True)
        wscale = 0.5 if mode == 'exact' else f32(1 / math.sqrt(C))
        Wn = (wscale * w.double())[None] * s.double()[:, None, :]
        return types.SimpleNamespace(w=w, s=s, wscale=wscale, rows=w), Wn, 2, wscale
    nw = 1 if c.api == 'thin_shared' else N
    W = fill(key + '/W', (nw, J, C), mode, 7)
    return types.SimpleNamespace(W=W, stride=0 if nw == 1 else J * C, rows=W), W.double().expand(N, J, C), 0, 1.0


# ------------------------------------------------------------------------------------------------------ case builders
def build_thin_fwd(c, mode):
    N, P, C, J = c.N, c.P, c.C, c.J
    x = fill(c.id + '/x', (N, P, C), mode, 7)
    ops, Wn, k, unit = weights(c, c.id, mode, N, J, C)
    ref = torch.einsum('npc,njc->njp', x.double(), Wn)
    S = torch.einsum('npc,njc->njp', x.double().abs(), Wn.abs())
    n = C
    bias = add = None
    if c.bias:
        bias = fill(c.id + '/bias', (J,), mode, 9, nonzero=True)
        ref, S, n = ref + bias.double()[None, :, None], S + bias.double().abs()[None, :, None], n + 1
    if c.add:
        add = fill(c.id + '/add', (N, J, P), mode, 50, nonzero=True)
        ref, S, n = ref + add.double(), S + add.double().abs(), n + 1
    self_check(mode, ref, S, unit, ops.rows)
    return types.SimpleNamespace(x=x, ops=ops, bias=bias, add=add, ref=ref, S=S, n=n, k=k)


def build_thin_bwdx(c, mode):
    N, P, C, J = c.N, c.P, c.C, c.J
    t = fill(c.id + '/t', (N, J, P), mode, 7)
    ops, Wn, k, unit = weights(c, c.id, mode, N, J, C)
    ref = torch.einsum('njp,njc->npc', t.double(), Wn)
    S = torch.einsum('njp,njc->npc', t.double().abs(), Wn.abs())
    n, old = J, None
    if c.acc:
        old = fill(c.id + '/old', (N, P, C), mode, 50, nonzero=True)
        ref, S, n = ref + old.double(), S + old.double().abs(), n + 1
    self_check(mode, ref, S, unit, ops.rows)
    return types.SimpleNamespace(t=t, ops=ops, old=old, ref=ref, S=S, n=n, k=k)


def build_thin_wgrad(c, mode):
    N, P, C, J = c.N, c.P, c.C, c.J
    t = fill(c.id + '/t', (N, J, P), mode, 3)
    x = fill(c.id + '/x', (N, P, C), mode, 3)
    ref = torch.einsum('njp,npc->njc', t.double(), x.double())
    S = torch.einsum('njp,npc->njc', t.double().abs(), x.double().abs())
    self_check(mode, ref, S)
    return types.SimpleNamespace(t=t, x=x, ref=ref, S=S, n=P, k=0)


def build_d_input(c, mode):
    """x = gain * lrelu(sum_j t_j W[j,c] + b[c]): J + 1 terms, then two more roundings (slope, gain): k = 2."""
    N, P, C, J = c.N, c.P, c.C, c.J
    t = fill(c.id + '/t', (N, J, P), mode, 7)
    W = fill(c.id + '/W', (J, C), mode, 7)
    b = fill(c.id + '/b', (C,), mode, 20, nonzero=True)
    slope, gain = (0.25, 2.0) if mode == 'exact' else (f32(0.2), f32(math.sqrt(2)))
    pre = torch.einsum('njp,jc->npc', t.double(), W.double()) + b.double()
    S = gain * (torch.einsum('njp,jc->npc', t.double().abs(), W.double().abs()) + b.double().abs())
    ref = torch.where(pre > 0, pre, pre * slope) * gain
    self_check(mode, ref, S, slope * gain, W)
    return types.SimpleNamespace(t=t, W=W, b=b, slope=slope, gain=gain, ref=ref, S=S, n=J + 1, k=2)


def build_chan_scale(c, mode):
    x = fill(c.id + '/x', (c.N, c.P, c.C), mode, 7)
    s = fill(c.id + '/s', (c.N, c.C), mode, 7, nonzero=True)
    ref = x.double() * s.double()[:, None, :]
    self_check(mode, ref, ref.abs())
    return types.SimpleNamespace(x=x, s=s, ref=ref, S=ref.abs(), n=1, k=0)


def divisor_for(c, mode):
    if mode == 'bound':
        return synth_tensor('forms/' + c.id + '/div', (c.N, c.C)).abs() + 0.5
    e = fill(c.id + '/dive', (c.N, c.C), mode, 1)                 # 2**{-1, 0, 1}, sign-mixed: the division is exact
    return torch.pow(2.0, e) * fill(c.id + '/divs', (c.N, c.C), mode, 1, nonzero=True)


def build_hw_dot(c, mode):
    """d[n,c] = sum_p a * r (/ divisor): P terms; the division is one more rounding of the result (k + 1).
    plain / scale: r = b (k = 0).  act: b holds y = gain * lrelu(z), r = lrelu^-1(y) - noise_w * noise[n,p] - bias[c], and
    the terms are the expanded products |a| * (|lrelu^-1 y| + |noise_w noise| + |bias|).  exact: gain = 2, slope = 0.25, the
    reciprocals and the un-activation multiply are exact.  bound: the model's gain = sqrt(2), slope = 0.2 (as fp32); the
    launcher rounds gain * slope and the reciprocal 1 / (gain * slope) (1 / gain: one rounding), the kernel rounds
    y * reciprocal and the two subtractions: at most 5 extra roundings on a term (the noise term: its product and the
    two subtractions), k = 5."""
    N, P, C = c.N, c.P, c.C
    a = fill(c.id + '/a', (N, P, C), mode, 3)
    b = fill(c.id + '/b', (N, P, C), mode, 6 if c.kind == 'act' else 3)
    out = types.SimpleNamespace(a=a, b=b, k=0, n=P, unit=1.0, div=None)
    r = R = b.double()
    if c.kind == 'act':
        out.slope, out.gain = (0.25, 2.0) if mode == 'exact' else (f32(0.2), f32(math.sqrt(2)))
        r = torch.where(r > 0, r / out.gain, r / (out.gain * out.slope))
        R = r.abs()
        out.bias = out.noise = out.nw = None
        if c.bias:
            out.bias = fill(c.id + '/bias', (C,), mode, 3, nonzero=True)
            r, R = r - out.bias.double(), R + out.bias.double().abs()
        if c.noise_nb:
            out.noise = fill(c.id + '/noise', (c.noise_nb, P), mode, 2)
            out.nw = torch.tensor([-2.0]) if mode == 'exact' else synth_tensor('forms/' + c.id + '/nw', (1,))
            nv = (float(out.nw) * out.noise.double()).expand(N, P)[:, :, None]
            r, R = r - nv, R + nv.abs()
        out.k, out.unit = 5 if mode == 'bound' else 0, 0.5
    out.ref = (a.double() * r).sum(1)
    out.S = (a.double().abs() * R.abs()).sum(1)
    self_check(mode, out.ref, out.S, out.unit)
    if c.div:
        out.div = divisor_for(c, mode)
        out.ref, out.S, out.k = out.ref / out.div.double(), out.S / out.div.double().abs(), out.k + 1
    if c.kind == 'scale':
        out.scale = fill(c.id + '/scale', (N, C), mode, 3, nonzero=True)
        out.scaled_ref = a.double() * out.scale.double()[:, None, :]
    return out


def build_add_scale(c, mode):
    a = fill(c.id + '/a', (c.n,), mode, 100)
    b = fill(c.id + '/b', (c.n,), mode, 100, nonzero=True) if c.b else None
    alpha = 0.5 if mode == 'exact' else f32(1 / math.sqrt(2))
    sm = a.double() + (b.double() if c.b else 0.0)
    S = (a.double().abs() + (b.double().abs() if c.b else 0.0)) * alpha
    self_check(mode, sm * alpha, S, alpha)
    return types.SimpleNamespace(a=a, b=b, alpha=alpha, ref=sm * alpha, S=S, n=2, k=1)     # the sum, then the product


# ------------------------------------------------------------------------------------------------------- case tables
def _fwd(form, api, N, C, P, J=3, bias=False, add=False, misalign=False, xmis=False):
    tag = f'{form[0]}{form[1]}x{form[2]}-{api}{"-bias" if bias else ""}{"-add" if add else ""}' \
          f'{"-add4B" if misalign else ""}{"-x4B" if xmis else ""}-N{N}-C{C}-P{P}-J{J}'
    return case(id='fwd-' + tag, form=form, api=api, N=N, C=C, P=P, J=J, bias=bias, add=add or misalign, misalign=misalign,
                xmis=xmis)


def _fwd_pair(form, N, C, P, J=3, misalign=False):
    """Every shape runs once as a plain per-sample product with `add` and once as the full ToRGB form."""
    return [_fwd(form, 'thin', N, C, P, J, add=True, misalign=misalign),
            _fwd(form, 'torgb', N, C, P, J, bias=True, add=True, misalign=misalign)]


def _fwd_variants(form, N, C, P):
    return [_fwd(form, 'thin', N, C, P), _fwd(form, 'thin_shared', N, C, P), _fwd(form, 'thin_shared', N, C, P, add=True),
            _fwd(form, 'torgb', N, C, P), _fwd(form, 'torgb', N, C, P, bias=True), _fwd(form, 'torgb', N, C, P, add=True)]


def _thin_fwd_cases():
    out = []
    for C in MFMA_C:
        mf = ('mfma', C // 16, 2 if C <= 128 else 1)
        lp = ('lpp',) + LPP_TABLE[C]
        # one 16-pixel group (three waves and the u = 1 slot idle) / group count not a multiple of waves x UNR / 64 x 64
        for P in (16, 80, 4096):
            out += _fwd_pair(mf, 1 if P == 16 else 3, C, P)
        out += _fwd_pair(lp, 3, C, 17 * 17)                          # P % 16 != 0
        out += _fwd_pair(lp, 3, C, 80, misalign=True)                # `add` 4 bytes off: the alignment test fails
    for C, (lpp, nq) in LPP_TABLE.items():
        blk = (256 // lpp) * 4                                       # pixels per block and UNR sweep
        for P in (blk - 1, blk, blk + 1, 3 * blk + 5):               # below / at / just above: the p < P clamp, the UNR tail
            out += _fwd_pair(('lpp', lpp, nq), 1 if P == blk else 3, C, P, misalign=C in MFMA_C and P % 16 == 0)
    for C in (4, 8, 36, 40):
        for P in (1, 63, 300):
            out += _fwd_pair(('generic', GENERIC_LPP[(C, 3)], 0), 3, C, P)
    for J in (1, 2, 3, 4):
        out += _fwd_pair(('mfma', 8, 2), 3, 128, 80, J)
        out += _fwd_pair(('lpp', 4, 4), 3, 64, 289, J)
        out += _fwd_pair(('lpp', 4, 6), 1, 96, 129, J)
        out += _fwd_pair(('generic', GENERIC_LPP[(8, J)], 0), 3, 8, 63, J)
    out += _fwd_pair(('generic', 1, 0), 3, 4, 63, 1)
    out += _fwd_variants(('mfma', 8, 2), 3, 128, 80) + _fwd_variants(('mfma', 16, 1), 1, 256, 48)
    out += _fwd_variants(('lpp', 4, 4), 3, 64, 289) + _fwd_variants(('generic', 8, 0), 3, 36, 63)
    # `x` itself 4 bytes off (every other operand aligned): no matrix-core form; the lanes-per-pixel and generic forms read
    # it with dword-aligned 16-byte loads and must give the same values
    out += [_fwd(('lpp', 8, 4), 'thin', 3, 128, 80, xmis=True), _fwd(('lpp', 8, 4), 'torgb', 3, 128, 80, bias=True, add=True, xmis=True),
            _fwd(('lpp', 4, 6), 'thin', 3, 96, 129, xmis=True), _fwd(('generic', 8, 0), 'torgb', 3, 36, 63, bias=True, xmis=True)]
    seen, uniq = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            uniq.append(c)
    return uniq


def _bwdx(api, N, C, P, J=3, note=''):
    form = thin_bwdx_form(C)
    return case(id=f'bwdx-{form}-{api}-N{N}-C{C}-P{P}-J{J}{note}', form=form, api=api.replace('_acc', ''), acc=api.endswith('_acc'),
                N=N, C=C, P=P, J=J)


def _thin_bwdx_cases():
    out = []
    for C in (16, 64, 128, 512, 1024):
        rows = 256 // (C // 4)
        # pixels per block at its floor of TB_UNR * rows: the TB_UNR = 4 loop runs zero times / exactly once and nothing is
        # left / once in block 0, then a second block of one pixel (remainder loop only) / three blocks, the last ragged
        for P, note in ((3 * rows, '-unr0'), (4 * rows, '-unr1'), (4 * rows + 1, '-unr1+1px'), (9 * rows + 3, '-ragged')):
            out += [_bwdx('thin', 3, C, P, note=note), _bwdx('torgb_acc', 3, C, P, note=note)]
        out += [_bwdx('torgb', 1, C, 9 * rows + 3), _bwdx('thin_shared', 3, C, 5 * rows - 1)]
    for api in ('thin', 'torgb', 'torgb_acc'):
        out.append(_bwdx(api, 4, 512, 64 * 64, note='-ppb16'))      # P N / 1024 = 16 pixels per block: two unrolled steps
        # pixels per block above the floor and not a multiple of TB_UNR * rows: a thread leaves the unrolled loop with
        # pixels left for the remainder loop (BWDX_HANDOFF: ppb and the (unrolled, remainder) steps it must show)
        for N, C, P in BWDX_HANDOFF:
            out.append(_bwdx(api, N, C, P, note='-handoff'))
    for C in (40, 48, 96):
        for P in (1, 27, 300):
            out += [_bwdx('thin', 3, C, P), _bwdx('torgb_acc', 3, C, P)]
        out += [_bwdx('torgb', 1, C, 300), _bwdx('thin_shared', 3, C, 27)]
    out += [_bwdx('thin', 1, 96, 256 * 256, note='-gridstride'), _bwdx('torgb_acc', 1, 96, 256 * 256, note='-gridstride')]
    for J in (1, 2, 4):
        out += [_bwdx('thin', 3, 64, 150, J), _bwdx('torgb_acc', 3, 64, 150, J), _bwdx('thin', 3, 48, 150, J),
                _bwdx('torgb_acc', 3, 48, 150, J)]
    return out


def _wgrad(N, C, P, J=3):
    return case(id=f'wgrad-nb{thin_wgrad_blocks(P)}-N{N}-C{C}-P{P}-J{J}', N=N, C=C, P=P, J=J, nb=thin_wgrad_blocks(P))


def _thin_wgrad_cases():
    # nb = 1 1 1 2 | 8 9 31 32 33 (thin_partial_sum_kernel's 4-way loop: b + 24 < nb, and its remainder) | 256 with the last
    # blocks past P (145 x 113: ppb = 65, blocks 253..255 are empty) | 256 x 256, the generator's largest map
    out = [_wgrad(3, 64, P) for P in (1, 63, 64, 65, 512, 576, 1984, 2048, 2112, 145 * 113, 256 * 256)]
    out += [_wgrad(1, 64, 576), _wgrad(1, 128, 256 * 256)]
    out += [_wgrad(3, 40, P) for P in (145, 2112)]                   # cg = 10, rpb = 25: threads 250..255 idle
    out += [_wgrad(3, 1028, P) for P in (145, 2112)]                 # ncol = 257: a second cbase pass with cg = 1
    out += [_wgrad(3, 64, 576, J) for J in (1, 2, 4)] + [_wgrad(3, 40, 145, J) for J in (1, 4)]
    return out


def _d_input_cases():
    out = [case(id=f'dinput-N{N}-C{C}-P{P}', N=N, C=C, P=P, J=3)
           for C in (64, 128, 256) for N, P in ((3, 37), (1, 4099))]                # P C / 4 not a multiple of 512
    out.append(case(id='dinput-gridcap-N1-C256-P66000', N=1, C=256, P=66000, J=3))   # above 8 192 blocks x 512 quads
    out += [case(id=f'dinput-N2-C64-P37-J{J}', N=2, C=64, P=37, J=J) for J in (1, 2, 4)]
    return out


def _chan_scale_cases():
    return [case(id='chanscale-vec-N3-C64-P35', N=3, C=64, P=35, off=0, vec=True),
            case(id='chanscale-vec-gridstride-N3-C64-P25000', N=3, C=64, P=25000, off=0, vec=True),
            case(id='chanscale-vec-N1-C1028-P17', N=1, C=1028, P=17, off=0, vec=True),
            case(id='chanscale-scalar-N3-C6-P35', N=3, C=6, P=35, off=0, vec=False),
            case(id='chanscale-scalar-x4B-N3-C64-P35', N=3, C=64, P=35, off=1, vec=False),
            case(id='chanscale-scalar-gridstride-N3-C6-P70001', N=3, C=6, P=70001, off=0, vec=False)]


def _hw_dot_cases():
    shapes = [(3, 64, P) for P in (1, 15, 16, 17, 8192, 8193, 65536)]      # 65 536: the 512-block cap, 128 rows per block
    shapes += [(3, 40, 17), (3, 40, 8193), (3, 512, 17), (1, 512, 8193), (3, 1028, 17), (1, 1028, 8193)]
    out = []
    for i, (N, C, P) in enumerate(shapes):
        sh = f'-N{N}-C{C}-P{P}'
        out += [case(id='hwdot-vec' + sh + ('-div' if i % 2 else ''), kind='dot', N=N, C=C, P=P, off=0, div=bool(i % 2)),
                case(id='hwdot-scalar-a4B' + sh + ('' if i % 2 else '-div'), kind='dot', N=N, C=C, P=P, off=1, div=not i % 2),
                case(id='hwdot-scale' + sh, kind='scale', N=N, C=C, P=P, off=0, div=False),
                case(id='hwdot-act-nonoise' + sh, kind='act', N=N, C=C, P=P, off=0, div=bool(i % 2), bias=True, noise_nb=0),
                case(id='hwdot-act-noise1' + sh, kind='act', N=N, C=C, P=P, off=0, div=not i % 2, bias=bool(i % 2), noise_nb=1),
                case(id='hwdot-act-noiseN' + sh, kind='act', N=N, C=C, P=P, off=0, div=False, bias=True, noise_nb=N)]
    for P in (1, 15, 16, 17, 8193, 65536):                                # C % 4 != 0: the scalar form on aligned operands
        out.append(case(id=f'hwdot-scalar-N3-C6-P{P}', kind='dot', N=3, C=6, P=P, off=0, div=P == 17))
    return out


def _add_scale_cases():
    return [case(id=f'addscale-n{n}-{"ab" if b else "a"}', n=n, b=b)
            for n in (4096, 4097, 1027, 3, 5_000_003) for b in (True, False)]      # n % 4 = 0 1 3 3 3; 5e6: grid-stride


THIN_FWD, THIN_BWDX, THIN_WGRAD, D_INPUT = _thin_fwd_cases(), _thin_bwdx_cases(), _thin_wgrad_cases(), _d_input_cases()
CHAN_SCALE, HW_DOT, ADD_SCALE = _chan_scale_cases(), _hw_dot_cases(), _add_scale_cases()


def params(cases):
    return pytest.mark.parametrize('c', cases, ids=[c.id for c in cases])


# ---------------------------------------------------------------------------------------------------- host-only tests
def test_lpp_table_matches_the_launcher_replay():
    for C, (lpp, nq) in LPP_TABLE.items():
        assert thin_fwd_form(C, 17, 3) == ('lpp', lpp, nq), C
    for C in range(4, 128, 4):
        if C not in LPP_TABLE:
            assert thin_fwd_form(C, 17, 3)[0] == 'generic', C
    for (C, J), lanes in GENERIC_LPP.items():
        assert thin_fwd_form(C, 17, J) == ('generic', lanes, 0), (C, J)
    reached = {c.form for c in THIN_FWD}
    assert {('mfma', 4, 2), ('mfma', 8, 2), ('mfma', 16, 1), ('mfma', 32, 1)} <= reached
    assert {('lpp',) + v for v in LPP_TABLE.values()} <= reached
    assert {nq for f, _, nq in reached if f == 'lpp'} == set(range(1, 9))
    assert {c.form for c in THIN_BWDX} == {'cols', 'fallback'}
    assert {c.nb for c in THIN_WGRAD} >= {1, 2, 8, 9, 31, 32, 33, 256}


def test_bwdx_column_owner_cases_run_the_loops_their_ids_name():
    """thin_bwdx_cols_kernel: the TB_UNR loop zero times, exactly once with nothing left, and — with more pixels per block
    than the floor — handing a thread over to a non-empty remainder loop, for the plain, ToRGB and accumulating entries."""
    handoff = set()
    for c in THIN_BWDX:
        if c.form != 'cols':
            continue
        rows = 256 // (c.C // 4)
        ppb, nbx, steps = thin_bwdx_plan(c.N, c.C, c.P)
        if '-unr0' in c.id:
            assert nbx == 1 and {u for u, _ in steps} == {0}, c.id
        elif '-unr1+1px' in c.id:
            assert nbx == 2 and steps == ({(1, 0), (0, 1), (0, 0)} if rows > 1 else {(1, 0), (0, 1)}), c.id
        elif '-unr1' in c.id:
            assert nbx == 1 and steps == {(1, 0)}, c.id
        elif '-ppb16' in c.id:
            assert ppb == 16 > 4 * rows and steps == {(2, 0)}, c.id
        elif '-handoff' in c.id:
            want_ppb, want_steps = BWDX_HANDOFF[(c.N, c.C, c.P)]
            assert (ppb, steps) == (want_ppb, want_steps) and ppb > 4 * rows and ppb % (4 * rows), c.id
            assert any(u > 0 and r > 0 for u, r in steps), c.id
            handoff.add((c.api, c.acc, c.C))
    assert handoff == {(api, acc, C) for api, acc in (('thin', False), ('torgb', False), ('torgb', True)) for C in (64, 128, 512)}


@pytest.mark.parametrize('builder,cases', [(build_thin_fwd, THIN_FWD), (build_thin_bwdx, THIN_BWDX), (build_thin_wgrad, THIN_WGRAD),
                                           (build_d_input, D_INPUT), (build_chan_scale, CHAN_SCALE), (build_hw_dot, HW_DOT),
                                           (build_add_scale, ADD_SCALE)],
                         ids=['thin_fwd', 'thin_bwdx', 'thin_wgrad', 'd_input', 'chan_scale', 'hw_dot', 'add_scale'])
def test_case_tables_are_exact_and_reach_their_form(builder, cases):
    """No device: every case's id names the form the replayed launcher picks, and its exact-mode inputs satisfy
    sum |terms| < 2**24 units with a non-constant result and distinct weight rows (asserted inside the builders)."""
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        if builder is build_thin_fwd:
            assert thin_fwd_form(c.C, c.P, c.J, aligned=not (c.misalign or c.xmis)) == c.form, c.id
        if builder is build_thin_wgrad:
            assert c.nb == thin_wgrad_blocks(c.P)
        if getattr(c, 'P', 0) * getattr(c, 'C', 0) > 1 << 21:        # the large maps: on the device run only (same builder)
            continue
        builder(c, 'exact')


# ----------------------------------------------------------------------------------------------------- device helpers
class Guarded:
    """numel floats between two sentinel bands; `off` floats of extra offset misalign the view by 4 * off bytes."""

    def __init__(self, numel, off=0, src=None):
        self.buf = torch.full((PAD + off + numel + PAD,), SENT, device=DEV, dtype=torch.float32)
        self.lo, self.hi = PAD + off, PAD + off + numel
        self.v = self.buf[self.lo:self.hi]
        assert self.v.data_ptr() % 16 == 4 * (off % 4)
        if src is not None:
            self.v.copy_(src.reshape(-1))

    def assert_bands(self, what):
        assert bool((self.buf[:self.lo] == SENT).all()) and bool((self.buf[self.hi:] == SENT).all()), f'{what}: wrote outside its buffer'


def dev_in(t, off=0):
    return None if t is None else Guarded(t.numel(), off, t)


def p(g):
    return None if g is None else g.v.data_ptr()


def stream():
    from rick_amd._lib import stream_ptr
    return stream_ptr()


def compare(c, mode, got, ref, S, n, k, what='out'):
    got = got.detach().cpu().reshape(ref.shape)
    if mode == 'exact':
        exp = ref.float()
        assert torch.equal(exp.double(), ref)
        bad = got != exp
        assert not bool(bad.any()), (f'{c.id} {what}: {int(bad.sum())} of {bad.numel()} elements differ, first at '
                                     f'{tuple(bad.nonzero()[0].tolist())}: {float(got[bad][0])} != {float(exp[bad][0])}')
    else:
        err = (got.double() - ref).abs()
        bound = (n + k) * U * S + 2.0 ** -23 * ref.abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f'{c.id} {what}: max |err| / bound = {worst:.3f} (n = {n}, k = {k})')
        assert bool((err <= bound).all()), f'{c.id} {what}: |err| up to {worst:.3f} x the a-priori bound'


def launch_weights(ops):
    if hasattr(ops, 'W'):
        return dev_in(ops.W), None
    return dev_in(ops.w), dev_in(ops.s)


# -------------------------------------------------------------------------------------------------------- GPU: thin
@gpu
@pytest.mark.parametrize('mode', MODES)
@params(THIN_FWD)
def test_thin_fwd_forms(c, mode):
    from rick_amd._lib import lib
    assert thin_fwd_form(c.C, c.P, c.J, aligned=not (c.misalign or c.xmis)) == c.form
    b = build_thin_fwd(c, mode)
    x, add, bias = dev_in(b.x, 1 if c.xmis else 0), dev_in(b.add, 1 if c.misalign else 0), dev_in(b.bias)
    wg, sg = launch_weights(b.ops)
    out = Guarded(c.N * c.J * c.P)
    if c.api == 'torgb':
        rc = lib.rick_torgb_fwd_f32(p(x), p(wg), p(sg), b.ops.wscale, p(bias), p(add), p(out), c.N, c.P, c.C, c.J, stream())
    else:
        rc = lib.rick_thin_fwd_f32(p(x), p(wg), b.ops.stride, p(add), p(out), c.N, c.P, c.C, c.J, stream())
    assert rc == 0
    torch.cuda.synchronize()
    out.assert_bands(c.id)
    compare(c, mode, out.v, b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(THIN_BWDX)
def test_thin_bwdx_forms(c, mode):
    from rick_amd._lib import lib
    b = build_thin_bwdx(c, mode)
    t = dev_in(b.t)
    wg, sg = launch_weights(b.ops)
    out = Guarded(c.N * c.P * c.C, src=b.old)       # ACC: pre-filled with `old`; otherwise every element still holds the sentinel
    if c.api == 'torgb':
        fn = lib.rick_torgb_bwdx_acc_f32 if c.acc else lib.rick_torgb_bwdx_f32
        rc = fn(p(t), p(wg), p(sg), b.ops.wscale, p(out), c.N, c.P, c.C, c.J, stream())
    else:
        assert not c.acc
        rc = lib.rick_thin_bwdx_f32(p(t), p(wg), b.ops.stride, p(out), c.N, c.P, c.C, c.J, stream())
    assert rc == 0
    torch.cuda.synchronize()
    out.assert_bands(c.id)
    compare(c, mode, out.v, b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(THIN_WGRAD)
def test_thin_wgrad_forms(c, mode):
    from rick_amd._lib import lib
    assert lib.rick_thin_wgrad_blocks(c.P) == c.nb
    b = build_thin_wgrad(c, mode)
    t, x = dev_in(b.t), dev_in(b.x)
    G, part = Guarded(c.N * c.J * c.C), Guarded(c.nb * c.N * c.J * c.C)
    rc = lib.rick_thin_wgrad_f32(p(t), p(x), p(G), c.N, c.P, c.C, c.J, p(part), stream())
    assert rc == 0
    torch.cuda.synchronize()
    G.assert_bands(c.id + ' G')
    part.assert_bands(c.id + ' partials')            # nothing past nb * N * J * C
    assert not bool((part.v == SENT).any()), 'a partial row was never written'
    compare(c, mode, G.v, b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(D_INPUT)
def test_d_input_forms(c, mode):
    from rick_amd._lib import lib
    b = build_d_input(c, mode)
    t, W, bias = dev_in(b.t), dev_in(b.W), dev_in(b.b)
    out = Guarded(c.N * c.P * c.C)
    rc = lib.rick_d_input_f32(p(t), p(W), p(bias), p(out), c.N, c.P, c.C, c.J, b.slope, b.gain, None, stream())
    assert rc == 0
    torch.cuda.synchronize()
    out.assert_bands(c.id)
    compare(c, mode, out.v, b.ref, b.S, b.n, b.k)


# ------------------------------------------------------------------------------------------------- GPU: elementwise
@gpu
@pytest.mark.parametrize('mode', MODES)
@params(CHAN_SCALE)
def test_chan_scale_forms(c, mode):
    from rick_amd._lib import lib
    assert c.vec == (c.C % 4 == 0 and c.off == 0)
    b = build_chan_scale(c, mode)
    x, s = dev_in(b.x, c.off), dev_in(b.s)
    out = Guarded(c.N * c.P * c.C)
    assert lib.rick_chan_scale_f32(p(x), p(s), p(out), c.N, c.P, c.C, stream()) == 0
    torch.cuda.synchronize()
    out.assert_bands(c.id)
    compare(c, mode, out.v, b.ref, b.S, b.n, b.k)


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(HW_DOT)
def test_hw_dot_forms(c, mode):
    from rick_amd._lib import lib
    nb = lib.rick_hw_dot_blocks(c.P)
    assert nb == hw_dot_blocks(c.P)
    b = build_hw_dot(c, mode)
    a, bb, div = dev_in(b.a, c.off), dev_in(b.b), dev_in(b.div)
    d, part = Guarded(c.N * c.C), Guarded(nb * c.N * c.C)
    scaled = None
    if c.kind == 'dot':
        rc = lib.rick_hw_dot_f32(p(a), p(bb), p(d), c.N, c.P, c.C, p(part), p(div), stream())
    elif c.kind == 'scale':
        sc, scaled = dev_in(b.scale), Guarded(c.N * c.P * c.C)
        rc = lib.rick_hw_dot_scale_f32(p(a), p(bb), p(d), p(sc), p(scaled), c.N, c.P, c.C, p(part), stream())
    else:
        bias, noise, nw = dev_in(b.bias), dev_in(b.noise), dev_in(b.nw)
        rc = lib.rick_hw_dot_act_f32(p(a), p(bb), p(d), c.N, c.P, c.C, p(bias), p(noise), p(nw), max(c.noise_nb, 1), b.slope, b.gain,
                                     p(part), p(div), stream())
    assert rc == 0
    torch.cuda.synchronize()
    d.assert_bands(c.id + ' d')
    part.assert_bands(c.id + ' partials')
    assert not bool((part.v == SENT).any()), 'a partial row was never written'
    compare(c, mode, d.v, b.ref, b.S, b.n, b.k)
    if scaled is not None:
        scaled.assert_bands(c.id + ' scaled')
        compare(c, mode, scaled.v, b.scaled_ref, b.scaled_ref.abs(), 1, 0, 'scaled')


@gpu
def test_hw_dot_scale_and_act_refuse_channel_counts_they_have_no_kernel_for():
    from rick_amd._lib import lib
    N, P, C = 2, 5, 6
    a, bb, d, s = (Guarded(n) for n in (N * P * C, N * P * C, N * C, N * C))
    sc, part = Guarded(N * P * C), Guarded(hw_dot_blocks(P) * N * C)
    assert lib.rick_hw_dot_scale_f32(p(a), p(bb), p(d), p(s), p(sc), N, P, C, p(part), stream()) == EINVAL
    assert lib.rick_hw_dot_act_f32(p(a), p(bb), p(d), N, P, C, None, None, None, 1, 0.25, 2.0, p(part), None, stream()) == EINVAL
    torch.cuda.synchronize()
    for g in (d, sc, part):
        assert bool((g.buf == SENT).all())


@gpu
@pytest.mark.parametrize('mode', MODES)
@params(ADD_SCALE)
def test_add_scale_forms(c, mode):
    from rick_amd._lib import lib
    b = build_add_scale(c, mode)
    a, bb = dev_in(b.a), dev_in(b.b)
    out = Guarded(c.n)
    assert lib.rick_add_scale_f32(p(a), p(bb), p(out), c.n, b.alpha, stream()) == 0
    torch.cuda.synchronize()
    out.assert_bands(c.id)
    compare(c, mode, out.v, b.ref, b.S, b.n, b.k)
