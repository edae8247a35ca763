"""Every form of the f32 GEMM convolution (inc_conv_kernel<NT, BWD, LIN>, rick_amd/csrc/inception.hip) and of the fully connected
layer (fc_partial_kernel<MT> / fc_reduce_kernel, rick_amd/csrc/vgg.hip), through the C ABI (rick_inc_conv_f32,
rick_inc_conv_bwd_f32, rick_inc_conv_lin_f32, rick_fc_f32, rick_fc_packed_floats, rick_fc_workspace_floats) on descriptors built
by rick_amd.gemm_conv.descriptor (by hand where a call must be refused), against the fp64 expressions of include/rick_hip.h as
tests/gemm_f64.py writes them out (F.conv2d / F.conv_transpose2d / F.linear in float64 on NCHW tensors; the packed layouts are
restated there, gemm_conv.pack / pack_transposed / fc.pack_fc_weight are not used):

    fwd   dst[s][m, c0[s] + col - seg_start[s]] = relu(sum_k A[m, k] wpk[k, col] + bias[col])
    bwd   dst[0][m, col] = (mask[m, col] > 0) ? sum_k A[m, k] wt[k, col] + add[m, col] : 0
    lin   dst[0][m, c0 + col] = act(sum_k A[m, k] wpk[k, col] + bias[col]) [+ res[m, c0 + col]],   act = identity | QuickGELU
    fc    out[m, n] = act(sum_k x[m, k] W[n, k] + bias[n]),   act = identity | ReLU

Every case states the form it reaches as a literal, which with a geometry tag is its id:

    conv<NT2,fwd>/seg3    conv<NT1,bwd>/mask+add    conv<NT2,lin2>/res-inplace    fc<MT2,scalar>/S8x33
    kernel instantiation / routed segments | epilogue operands | residual | slices x k blocks per slice

and the host-only test replays the dispatch (the column block, the act arm of rick_inc_conv_lin_f32, MT from M <= 32, vec from
K % 4 and the alignment of x, fc_plan), holds the literals to the replay and the replay to the library, and asserts that all
eight conv instantiations and all four fc forms are reached, fc with one slice, with several and with a short last slice.

Checks, none with a measured tolerance but QuickGELU's:

  exact  operands, bias, add and res non-zero integers |v| <= 4 of mixed sign, masks integers in [-2, 2] (zeros included), and
         sum |terms| < 2**24 for every output (asserted on the CPU): every product and every partial sum in any order, through the
         fc chains and slice sums, is an exact fp32 number, so the result is torch.equal to the fp64 one cast to fp32.  Pins taps,
         halos, stride and padding arithmetic, K and row tails, column routing, the mask rule and the fc k-block rotation.
  bound  standard-normal operands (weights scaled by K**-0.5, bias by 0.1); per element
             |dev - ref64| <= (K + R) * 2**-24 * (sum |x||w| + |bias| + |add or res|) + 2**-23 |ref|
         R counts the further roundings on a term.  Conv (R = 3): v_mfma_f32_32x32x2_f32 rounds a product and the addition onto
         the accumulator (K additions are the K of the bound; 1 for a product rounded on its own), the epilogue adds the bias or
         `add` (1) and the residual (1); ReLU, the mask and the stores round nothing.  fc (R = 3 + S): the product (1), the add of
         the even and the odd chain (1), S - 1 slice adds and the bias (S), the activation none.  A masked-off element must be an
         exact zero.  Each bound case is launched twice: bit-identical.
  QuickGELU (LIN = 2), the one inexact step (expf).  exact mode: the output is bit-equal to rick_clip_quickgelu_f32 of the
         LIN = 1 output of the same case (which is itself equal to fp64), the residual added as one fp32 add on the CPU.  bound
         mode: max |d| / max |ref| within FACTOR = 4 x the same figure of the fp32 torch-CPU composition against fp64
         (QGELU_CPU_BASE, measured on the CPU against the reference, never against the kernel), as tests/test_gpu_clip.py does.

Every device case: destinations and the fc workspace between sentinel bands, channels of a destination outside
[c0, c0 + ncols) keep the sentinel bit for bit; every operand (in, wpk with its Kp tail rows, bias, add, res, the fc x and packed
weight) is a view into a NaN-fenced buffer, `mask` into a +inf-fenced one (it only passes through a comparison), a residual's
channels outside the slice are NaN; a refused call returns 22 and leaves every output untouched.

Invariants (torch.equal, bound-mode data), on every conv case they apply to: bn = 64 and bn = 128 give the same bits; the last
image alone gives the bits it has inside the batch; routed segments give the bits of the unrouted GEMM; the in-place residual
gives the bits of the separate one.  fc: rows alone (M = 1, 32, 33) against M = 64; x misaligned by 1 - 3 floats (scalar staging)
against aligned x (vec).

One case poisons the input pixels that no tap of any output reads (the row and column a stride-2 floor leaves over) with NaN:
the zero rows of wpk beyond K do not make a read at k >= K harmless (0 * NaN), the k < K predicate does.

Forms no small geometry reaches: none.  All eight conv instantiations and the four fc forms have cases here."""
import functools
import types

import pytest
import torch

from tests import gemm_f64 as G
from tests.forms_common import DEV, SENT, Fenced, Guarded, _gen, fenced, ints, p, stream

gpu = pytest.mark.gpu
EINVAL = 22
R_CONV = 3                    # further roundings on a term (module docstring)
R_FC = 3                      # + S
FACTOR = 4
INF = float('inf')
# max |fp32 torch CPU - ref64| / max |ref64| of act(conv(x) + b) [+ res], act = QuickGELU, on conv_data(id, 'bound'); keyed
# (geometry tag, with res).  python -c "from tests.test_gpu_gemm_forms import quickgelu_cpu_bases as f; f()"
QGELU_CPU_BASE = {('M129-K72-Co65', False): 3.093e-07, ('M129-K72-Co65', True): 2.277e-07,
                  ('M257-K36-Co33', False): 1.698e-07, ('M257-K36-Co33', True): 1.524e-07,
                  ('M12-K64-Co64', False): 3.397e-07, ('M12-K64-Co64', True): 2.177e-07}


def case(**kw):
    return types.SimpleNamespace(**kw)


# ------------------------------------------------------------------------------------------------------------- cases
S1, S2 = (1, 1), (2, 2)


def _conv(want, tag, kind, n, h, w, ci, k, s, pad, segs, bn=None, **kw):
    co = sum(sg[3] for sg in segs)
    c = case(want=want, tag=tag, id=f'{want}/{tag}', kind=kind, n=n, h=h, w=w, ci=ci, k=k, s=s, p=pad, segs=segs, co=co,
             bn=bn or G.column_block(co), act=0, res=None, mask=False, add=False, zero_ch3=False, poison=False, cin=co)
    c.__dict__.update(kw)
    return c


def _fwd(want, tag, n, h, w, ci, k, s, pad, co, bn=None, **kw):
    segs = co if isinstance(co, list) else [(0, co, 0, co)]
    return _conv(want, tag, 'fwd', n, h, w, ci, k, s, pad, segs, bn, **kw)


# (destination, ldc, c0, ncols): every boundary of (5, 30, 1, 28) inside one 32-column group; InceptionA's heads (64 | 48 | 64);
# four segments on three destinations, one shared at two c0, with ldc > c0 + ncols
SEG_5_30_1_28 = [(0, 5, 0, 5), (1, 40, 7, 30), (2, 4, 2, 1), (3, 28, 0, 28)]
SEG_INCEPTION_A = [(0, 64, 0, 64), (1, 64, 16, 48), (2, 64, 0, 64)]
SEG_SHARED = [(0, 20, 0, 20), (1, 100, 3, 45), (2, 40, 4, 33), (1, 100, 60, 32)]

FWD = [
    _fwd('conv<NT1,fwd>/seg1', 'M128-K4-Co1', 128, 1, 1, 4, (1, 1), S1, (0, 0), 1),
    _fwd('conv<NT1,fwd>/seg1', 'M129-K36-Co33', 43, 3, 5, 4, (3, 3), S1, (0, 0), 33),                 # 1 x 3 outputs per image
    _fwd('conv<NT1,fwd>/seg1', 'M127-K60-Co64', 127, 3, 5, 4, (3, 5), S1, (0, 0), 64),                # the kernel is the image
    _fwd('conv<NT1,fwd>/seg1', 'M126-K72-Co3', 2, 7, 9, 8, (3, 3), S1, (1, 1), 3),
    _fwd('conv<NT2,fwd>/seg1', 'M126-K288-Co65', 2, 7, 9, 32, (3, 3), S1, (1, 1), 65),
    _fwd('conv<NT1,fwd>/seg1', 'M189-K28-Co130-k1x7', 3, 7, 9, 4, (1, 7), S1, (0, 3), 130),
    _fwd('conv<NT2,fwd>/seg1', 'M189-K28-Co130-k1x7', 3, 7, 9, 4, (1, 7), S1, (0, 3), 130, bn=128),
    _fwd('conv<NT2,fwd>/seg1', 'M30-K28-Co64-k7x1', 2, 3, 5, 4, (7, 1), S1, (3, 0), 64, bn=128),      # padding as wide as the image
    _fwd('conv<NT1,fwd>/seg1', 'M315-K100-Co33-k5x5', 5, 7, 9, 4, (5, 5), S1, (2, 2), 33),
    _fwd('conv<NT2,fwd>/seg1', 'M36-K72-Co65-s2p0', 3, 7, 9, 8, (3, 3), S2, (0, 0), 65),
    _fwd('conv<NT1,fwd>/seg1', 'M60-K36-Co33-s2p1', 3, 7, 9, 4, (3, 3), S2, (1, 1), 33),
    _fwd('conv<NT1,fwd>/seg1', 'M45-K36-Co33-p2-on-1x1', 5, 1, 1, 4, (3, 3), S1, (2, 2), 33),         # every tap but one is padding
    _fwd('conv<NT1,fwd>/seg1', 'M12-K64-Co64-patch', 3, 8, 8, 4, (4, 4), (4, 4), (0, 0), 64, zero_ch3=True),
    _fwd('conv<NT2,fwd>/seg1', 'M31-K4096-Co65', 31, 1, 1, 4096, (1, 1), S1, (0, 0), 65),
    _fwd('conv<NT1,fwd>/seg1', 'M257-K60-Co33', 257, 3, 5, 4, (3, 5), S1, (0, 0), 33),
    _fwd('conv<NT2,fwd>/seg1', 'M1-K36-Co65', 1, 1, 1, 4, (3, 3), S1, (1, 1), 65),
    _fwd('conv<NT1,fwd>/seg1', 'M36-K36-Co33-s2p0-poisoned', 3, 8, 10, 4, (3, 3), S2, (0, 0), 33, poison=True),
    _fwd('conv<NT1,fwd>/seg4', 'M126-K72-Co64-5+30+1+28', 2, 7, 9, 8, (3, 3), S1, (1, 1), SEG_5_30_1_28),
    _fwd('conv<NT2,fwd>/seg4', 'M126-K72-Co64-5+30+1+28', 2, 7, 9, 8, (3, 3), S1, (1, 1), SEG_5_30_1_28, bn=128),
    _fwd('conv<NT1,fwd>/seg3', 'M126-K72-Co176-64+48+64', 2, 7, 9, 8, (3, 3), S1, (1, 1), SEG_INCEPTION_A),
    _fwd('conv<NT1,fwd>/seg4', 'M189-K28-Co130-shared', 3, 7, 9, 4, (1, 7), S1, (0, 3), SEG_SHARED),
    _fwd('conv<NT2,fwd>/seg4', 'M189-K28-Co130-shared', 3, 7, 9, 4, (1, 7), S1, (0, 3), SEG_SHARED, bn=128),
]

# the data gradient: H x W and the images that make M % 128 = 1 or 127; (Ci, Co) of the descriptor = (the forward's output
# channels, its input channels), (64, 4) the NHWC4 image gradient (3 channels travel as 4: column 3 of the operand is zero)
BWD_HW = [(1, 1, 129), (3, 5, 17), (9, 5, 37)]                      # M = 129, 255, 1665
BWD_CH = [(64, 4, 64), (8, 64, 128), (68, 36, 64)]                  # (Ci, Co, bn)
BWD = []
for _h, _w, _n in BWD_HW:
    for _ci, _co, _bn in BWD_CH:
        for _mask in (False, True):
            for _add in (False, True):
                _epi = '+'.join([nm for nm, on in (('mask', _mask), ('add', _add)) if on]) or 'plain'
                BWD.append(_conv(f'conv<NT{_bn // 64},bwd>/{_epi}', f'M{_n * _h * _w}-K{9 * _ci}-Co{_co}-{_h}x{_w}', 'bwd', _n, _h, _w,
                                 _ci, (3, 3), S1, (1, 1), [(0, _co, 0, _co)], _bn, mask=_mask, add=_add, cin=3 if _co == 4 else _co))

# the linear epilogue into channels [5, 5 + Co) of Co + 13: rows of K, and the CLIP patch geometry (4 x 4 stride 4, channel 3 zero)
LIN_GEOM = [('M129-K72-Co65', 129, 1, 1, 72, (1, 1), S1, 65, False), ('M257-K36-Co33', 257, 1, 1, 36, (1, 1), S1, 33, False),
            ('M12-K64-Co64', 3, 8, 8, 4, (4, 4), (4, 4), 64, True)]
LIN = []
for _tag, _n, _h, _w, _ci, _k, _s, _co, _z in LIN_GEOM:
    for _act in (0, 1):
        for _res in (None, 'separate', 'inplace'):
            LIN.append(_conv(f"conv<NT{G.column_block(_co) // 64},lin{1 + _act}>/res-{_res or 'none'}", _tag, 'lin', _n, _h, _w, _ci, _k, _s,
                             (0, 0), [(0, _co + 13, 5, _co)], act=_act, res=_res, zero_ch3=_z))

CONV = FWD + BWD + LIN
CONV_BY_ID = {c.id: c for c in CONV}
assert len(CONV_BY_ID) == len(CONV)


def _fc(want, M, K, N, relu, off=0):
    return case(want=want, id=f'{want}/M{M}-K{K}-N{N}-relu{relu}-off{off}', M=M, K=K, N=N, relu=relu, off=off)


FC = [
    _fc('fc<MT1,scalar>/S1x1', 1, 1, 1, 0),
    _fc('fc<MT1,scalar>/S1x1', 32, 7, 31, 1),
    _fc('fc<MT2,vec>/S1x1', 33, 8, 32, 0),
    _fc('fc<MT2,scalar>/S1x8', 64, 63, 127, 1),                      # a stage of 8 k blocks, the last k missing
    _fc('fc<MT1,vec>/S1x8', 1, 64, 128, 1),
    _fc('fc<MT2,scalar>/S2x32', 33, 510, 129, 0),
    _fc('fc<MT1,vec>/S2x32', 32, 512, 200, 1),
    _fc('fc<MT2,vec>/S8x33', 64, 2056, 200, 0),                      # 257 k blocks: seven slices of 33 and one of 26; stage tail of 1
    _fc('fc<MT1,vec>/S8x33', 1, 2056, 31, 1),
    _fc('fc<MT2,scalar>/S2x32', 64, 512, 1, 0, off=1),
    _fc('fc<MT1,scalar>/S1x8', 32, 64, 129, 1, off=3),
    _fc('fc<MT2,scalar>/S8x33', 33, 2056, 127, 1, off=2),
]
FC_BY_ID = {c.id: c for c in FC}
assert len(FC_BY_ID) == len(FC)


# -------------------------------------------------------------------------------------------------------------- data
def geometry(c, n=None):
    oh, ow = G.out_hw(c.h, c.w, c.k, c.s, c.p)
    return oh, ow, (c.n if n is None else n) * oh * ow, c.k[0] * c.k[1] * c.ci


@functools.lru_cache(maxsize=None)
def conv_data(cid, mode):
    """The operands of a case on the CPU, the fp64 result [M, Co] and S = sum |x||w| per output; computed once per (case, mode)."""
    c = CONV_BY_ID[cid]
    oh, ow, M, K = geometry(c)
    key = f'{c.kind}/{c.tag}/{mode}'          # cases of one geometry share operands: epilogue arms and blocks compare bit for bit
    shape_w = (c.ci, c.co, 3, 3) if c.kind == 'bwd' else (c.co, c.ci) + c.k
    if mode == 'exact':
        x, w, bias = ints(key + 'x', (c.n, c.h, c.w, c.ci), 4), ints(key + 'w', shape_w, 4), ints(key + 'b', (c.co,), 4)
        extra = ints(key + 'e', (M, c.co), 4)
        mask = torch.randint(-2, 3, (M, c.co), generator=_gen(key + 'm')).float()
    else:
        g = _gen(key)
        x, w = torch.randn(c.n, c.h, c.w, c.ci, generator=g), torch.randn(shape_w, generator=g) * K ** -0.5
        bias, extra, mask = torch.randn(c.co, generator=g) * 0.1, torch.randn(M, c.co, generator=g), torch.randn(M, c.co, generator=g)
    if c.zero_ch3:
        x[..., 3] = 0
    if c.kind == 'bwd':
        w[:, c.cin:] = 0                                               # the image's 3 channels travel as 4
    d = case(x=x, w=w, bias=bias, extra=None, mask=None, xdev=x)
    if c.poison:                                                       # pixels outside every window: the reference never sees them
        assert c.s == S2 and c.p == (0, 0) and (c.h - c.k[0]) % 2 == 1 and (c.w - c.k[1]) % 2 == 1
        d.xdev = x.clone()
        d.xdev[:, -1], d.xdev[:, :, -1] = float('nan'), float('nan')
        x = x.clone()
        x[:, -1], x[:, :, -1] = 0, 0
    if c.kind == 'fwd':
        d.pre = G.conv_f64(x, w, bias, c.s, c.p)
        d.ref, d.S = d.pre.clamp_min(0), G.conv_f64(x.abs(), w.abs(), bias.abs(), c.s, c.p)
    elif c.kind == 'lin':
        d.extra = extra if c.res else None
        d.pre = G.conv_f64(x, w, bias, c.s, c.p)
        d.ref = G.conv_lin_f64(x, w, bias, c.s, c.p, c.act, d.extra)
        d.S = G.conv_f64(x.abs(), w.abs(), bias.abs(), c.s, c.p) + (extra.abs().double() if c.res else 0)
    else:
        d.extra, d.mask = extra if c.add else None, mask if c.mask else None
        d.ref = G.conv_bwd_f64(x, w, d.mask, d.extra)
        d.S = G.conv_bwd_f64(x.abs(), w.abs(), None, extra.abs() if c.add else None)
    assert d.ref.shape == (M, c.co)
    return d


@functools.lru_cache(maxsize=None)
def conv_operand(cid, mode, bn):
    c, d = CONV_BY_ID[cid], conv_data(cid, mode)
    if c.kind == 'bwd':
        wt = G.pack_wt(d.w, bn)
        return wt, torch.zeros(wt.shape[1])
    return G.pack_wpk(d.w, bn, d.bias)


@functools.lru_cache(maxsize=None)
def fc_data(cid, mode):
    c = FC_BY_ID[cid]
    key = f'fc/{c.M}/{c.K}/{c.N}/{mode}'
    if mode == 'exact':
        x, w, b = ints(key + 'x', (c.M, c.K), 4), ints(key + 'w', (c.N, c.K), 4), ints(key + 'b', (c.N,), 4)
    else:
        g = _gen(key)
        x, w, b = torch.randn(c.M, c.K, generator=g), torch.randn(c.N, c.K, generator=g) * c.K ** -0.5, torch.randn(c.N, generator=g) * 0.1
    return case(x=x, w=w, b=b, wpk=G.pack_fc(w), ref=G.fc_f64(x, w, b, c.relu), S=G.fc_f64(x.abs(), w.abs(), b.abs(), 0))


def conv_bound(c, d):
    K = geometry(c)[3]
    return (K + R_CONV) * 2.0 ** -24 * d.S + 2.0 ** -23 * d.ref.abs()


def fc_bound(c, d):
    return (c.K + R_FC + G.fc_plan(c.K, c.N)[0]) * 2.0 ** -24 * d.S + 2.0 ** -23 * d.ref.abs()


def max_rel_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def quickgelu_cpu_bases():
    """Prints QGELU_CPU_BASE: the fp32 torch-CPU composition against the fp64 reference, on the CPU alone."""
    for c in LIN:
        if c.act and c.res != 'inplace':
            d = conv_data(c.id, 'bound')
            err = max_rel_err(G.conv_lin_f32(d.x, d.w, d.bias, c.s, c.p, 1, d.extra), d.ref)
            print(f"('{c.tag}', {c.res is not None}): {err:.3e},")


# ------------------------------------------------------------------------------------------------------- host-only test
def test_literals_replay_and_coverage():
    from rick_amd._lib import lib
    from rick_amd import gemm_conv
    reached = set()
    for c in CONV:
        oh, ow, M, K = geometry(c)
        co = sum(sg[3] for sg in c.segs)
        form = G.conv_form(c.kind, c.bn, c.act)
        tail = {'fwd': f'seg{len(c.segs)}', 'lin': f"res-{c.res or 'none'}",
                'bwd': '+'.join([nm for nm, on in (('mask', c.mask), ('add', c.add)) if on]) or 'plain'}[c.kind]
        assert c.want == f'{form}/{tail}', c.id
        assert c.tag.startswith(f'M{M}-K{K}-Co{co}'), c.id
        assert c.bn in (64, 128) and G.column_block(co) == gemm_conv.column_block(co)
        assert c.ci % 4 == 0 and oh > 0 and ow > 0
        reached.add(form)
        for mode in ('exact', 'bound'):
            d = conv_data(c.id, mode)
            assert bool(torch.isfinite(d.ref).all()) and bool(torch.isfinite(d.S).all())
        d = conv_data(c.id, 'exact')
        assert float(d.S.max()) < 2 ** 24, c.id                         # every partial sum is an exact fp32 number
        assert not bool((d.ref.float() == SENT).any()), c.id
        if c.kind == 'fwd':
            clipped = float((d.pre < 0).double().mean())
            assert 0.2 <= clipped <= 0.8, (c.id, clipped)
        if c.mask:
            off = float((d.mask <= 0).double().mean())
            assert 0.25 <= off <= 0.75 and bool((d.mask == 0).any()) and bool((d.mask < 0).any()), (c.id, off)
        for di in {sg[0] for sg in c.segs}:                              # segments of one destination share ldc and do not overlap
            mine = [sg for sg in c.segs if sg[0] == di]
            cols = [ch for sg in mine for ch in range(sg[2], sg[2] + sg[3])]
            assert len({sg[1] for sg in mine}) == 1 and len(set(cols)) == len(cols) and max(cols) < mine[0][1]
    assert reached == set(G.CONV_FORMS), sorted(set(G.CONV_FORMS) - reached)
    assert {c.tag for c in LIN if c.act} == {t for t, _ in QGELU_CPU_BASE}

    forms, slices = set(), set()
    for c in FC:
        S, kbs = G.fc_plan(c.K, c.N)
        form = G.fc_form(c.M, c.K, c.off)
        assert c.want == f'{form}/S{S}x{kbs}', (c.id, f'{form}/S{S}x{kbs}')
        assert lib.rick_fc_workspace_floats(c.M, c.K, c.N) == G.fc_workspace_floats(c.M, c.K, c.N) == S * c.M * c.N
        d = fc_data(c.id, 'exact')
        assert lib.rick_fc_packed_floats(c.K, c.N) == G.fc_packed_floats(c.K, c.N) == d.wpk.numel()
        assert float(d.S.max()) < 2 ** 24 and not bool((d.ref.float() == SENT).any())
        if c.relu:
            pre = G.fc_f64(d.x, d.w, d.b, 0)
            assert 0.2 <= float((pre < 0).double().mean()) <= 0.8, c.id
        forms.add(form)
        KB = G.cdiv(c.K, G.FC_KB)
        slices.add('one' if S == 1 else 'short-last' if KB % kbs else 'several')
        if (KB - (S - 1) * kbs) % G.FC_CH:
            slices.add('stage-tail')
    assert forms == set(G.FC_FORMS)
    assert slices == {'one', 'several', 'short-last', 'stage-tail'}
    assert {c.M for c in FC} == {1, 32, 33, 64} and {c.K for c in FC} == {1, 7, 8, 63, 64, 510, 512, 2056}
    assert {c.N for c in FC} == {1, 31, 32, 127, 128, 129, 200} and {c.relu for c in FC} == {0, 1}
    for bad in ((65, 8, 8), (0, 8, 8), (1, 0, 8), (1, 8, 0), (1, (1 << 24) + 1, 8), (1, 8, (1 << 20) + 1)):
        assert lib.rick_fc_workspace_floats(*bad) == -1
    assert lib.rick_fc_packed_floats(0, 8) == lib.rick_fc_packed_floats(8, 0) == -1


def test_packed_layouts_against_the_host_packers():
    """The restated layouts and the project's packers agree (both are needed: the tests never launch on the project's own)."""
    from rick_amd import gemm_conv
    from rick_amd.fc import pack_fc_weight
    w = ints('layout/w', (5, 8, 3, 2), 4)
    for bn in (64, 128):
        assert torch.equal(G.pack_wpk(w, bn)[0], gemm_conv.pack(w, bn=bn)[0])
    w3 = ints('layout/w3', (8, 3, 3, 3), 4)
    assert torch.equal(G.pack_wt(w3, 64), gemm_conv.pack_transposed(w3)[0])
    wf = ints('layout/fc', (130, 13), 4)
    assert torch.equal(G.pack_fc(wf), pack_fc_weight(wf))


# ---------------------------------------------------------------------------------------------------------- launches
def launch_conv(c, d, ops, bn, img=None, segs=None, res='case', act=None):
    """One launch of a case on fenced operands and guarded destinations -> the GEMM result [M, Co] on the CPU, gathered from the
    destinations.  img: that image alone; segs: another routing; res: another residual mode; act: another activation."""
    from rick_amd import gemm_conv
    from rick_amd._lib import lib
    x = d.xdev if img is None else d.xdev[img:img + 1]
    oh, ow, M, _ = geometry(c, x.shape[0])
    rows = slice(0, M) if img is None else slice(img * oh * ow, (img + 1) * oh * ow)
    segs, res = segs or c.segs, c.res if res == 'case' else res
    wpk, bias = ops
    fx, fw, fb = fenced(x), fenced(wpk), fenced(bias)
    dests = {}
    for di, ldc, _, _ in segs:
        if di not in dests:
            dests[di] = Guarded(M * ldc)
    a = gemm_conv.descriptor(x.shape[0], c.h, c.w, c.ci, c.k, c.s, c.p, wpk.shape[1], bn, [(p(dests[di]), ldc, c0, nc) for di, ldc, c0, nc in segs])
    keep = [fx, fw, fb]
    if c.kind == 'fwd':
        rc = lib.rick_inc_conv_f32(p(fx), p(fw), p(fb), a, stream())
    elif c.kind == 'bwd':
        fm, fa = fenced(None if d.mask is None else d.mask[rows], fill=INF), fenced(None if d.extra is None else d.extra[rows])
        keep += [fm, fa]
        rc = lib.rick_inc_conv_bwd_f32(p(fx), p(fw), p(fm), p(fa), a, stream())
    else:
        (_, ldc, c0, nc), = segs
        rp = None
        if res == 'separate':                                           # laid out like the destination; NaN outside the slice
            full = torch.full((M, ldc), float('nan'))
            full[:, c0:c0 + nc] = d.extra[rows]
            keep.append(fenced(full))
            rp = p(keep[-1])
        elif res == 'inplace':
            dests[0].v.view(M, ldc)[:, c0:c0 + nc] = d.extra[rows].to(DEV)
            rp = p(dests[0])
        rc = lib.rick_inc_conv_lin_f32(p(fx), p(fw), p(fb), rp, c.act if act is None else act, a, stream())
    assert rc == 0, f'{c.id}: status {rc}'
    torch.cuda.synchronize()
    out, col = torch.empty(M, sum(sg[3] for sg in segs)), 0
    host = {di: gd.v.view(M, -1).cpu() for di, gd in dests.items()}
    named = {di: torch.zeros(v.shape[1], dtype=torch.bool) for di, v in host.items()}
    for di, ldc, c0, nc in segs:
        out[:, col:col + nc] = host[di][:, c0:c0 + nc]
        named[di][c0:c0 + nc] = True
        col += nc
    for di, gd in dests.items():
        gd.assert_bands(f'{c.id} destination {di}')
        assert bool((host[di][:, ~named[di]] == SENT).all()), f'{c.id}: destination {di} written outside its channel slices'
    return out


def quickgelu_dev(u):
    from rick_amd._lib import lib
    src, dst = fenced(u), Guarded(u.numel())
    assert lib.rick_clip_quickgelu_f32(p(src), p(dst), u.numel(), stream()) == 0
    torch.cuda.synchronize()
    dst.assert_bands('rick_clip_quickgelu_f32')
    return dst.v.cpu().view(u.shape)


def hold_to_bound(what, got, ref, bound, zero=None):
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all()), f'{what}: non-finite output'
    ratio = err / bound.clamp_min(1e-300)
    i = int(ratio.argmax())
    print(f'{what} bound: max |d| {float(err.max()):.3e}, worst |d| / bound {float(ratio.reshape(-1)[i]):.3f} '
          f'(|d| {float(err.reshape(-1)[i]):.3e} against {float(bound.reshape(-1)[i]):.3e})')
    assert bool((err <= bound).all()), f'{what}: {int((err > bound).sum())} elements beyond the bound'
    if zero is not None:
        assert bool((got[zero] == 0).all()), f'{what}: a masked-off element is not an exact zero'


@gpu
@pytest.mark.parametrize('cid', list(CONV_BY_ID))
def test_conv_case(cid):
    c = CONV_BY_ID[cid]
    run = lambda mode, bn=c.bn, **kw: launch_conv(c, conv_data(cid, mode), conv_operand(cid, mode, bn), bn, **kw)
    d = conv_data(cid, 'exact')
    got = run('exact')
    if c.kind == 'lin' and c.act:
        u = run('exact', res=None, act=0)
        assert torch.equal(u, d.pre.float()), f'{cid}: the LIN = 1 output is not the fp64 one'
        want = quickgelu_dev(u)
        if c.res:
            want = want + d.extra
        assert torch.equal(got, want), f'{cid}: LIN = 2 is not rick_clip_quickgelu_f32 of LIN = 1 [+ res]'
        print(f'{cid} exact: equal (to rick_clip_quickgelu_f32 of the LIN = 1 output, itself equal to fp64)')
    else:
        bad = got != d.ref.float()
        assert not bool(bad.any()), f'{cid}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}'
        print(f'{cid} exact: equal')

    d = conv_data(cid, 'bound')
    got = run('bound')
    if c.kind == 'lin' and c.act:
        err, base = max_rel_err(got, d.ref), QGELU_CPU_BASE[(c.tag, c.res is not None)]
        print(f'{cid} bound: max |d| / max |ref| {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
        assert err <= FACTOR * base
    else:
        hold_to_bound(cid, got, d.ref, conv_bound(c, d), None if d.mask is None else d.mask <= 0)
    assert torch.equal(run('bound'), got), f'{cid}: two launches differ'
    assert torch.equal(run('bound', bn=192 - c.bn), got), f'{cid}: bn = 64 and bn = 128 differ'
    if c.n > 1:
        oh, ow, _, _ = geometry(c)
        assert torch.equal(run('bound', img=c.n - 1), got[(c.n - 1) * oh * ow:]), f'{cid}: an image alone differs from the batch'
    if len(c.segs) > 1:
        assert torch.equal(run('bound', segs=[(0, c.co, 0, c.co)]), got), f'{cid}: routed segments differ from the unrouted GEMM'
    if c.res == 'inplace':
        assert torch.equal(run('bound', res='separate'), got), f'{cid}: the in-place residual differs from the separate one'


def launch_fc(c, d, rows=None, off=None):
    from rick_amd._lib import lib
    x = d.x if rows is None else d.x[rows]
    M, off = x.shape[0], c.off if off is None else off
    fx, fw, fb = fenced(x, off), fenced(d.wpk), fenced(d.b)
    ws, out = Guarded(lib.rick_fc_workspace_floats(M, c.K, c.N)), Guarded(M * c.N)
    rc = lib.rick_fc_f32(p(fx), p(fw), p(fb), p(ws), p(out), M, c.K, c.N, c.relu, stream())
    assert rc == 0, f'{c.id}: status {rc}'
    torch.cuda.synchronize()
    ws.assert_bands(f'{c.id} workspace')
    out.assert_bands(f'{c.id} output')
    return out.v.cpu().view(M, c.N)


@gpu
@pytest.mark.parametrize('cid', list(FC_BY_ID))
def test_fc_case(cid):
    c = FC_BY_ID[cid]
    d = fc_data(cid, 'exact')
    bad = launch_fc(c, d) != d.ref.float()
    assert not bool(bad.any()), f'{cid}: {int(bad.sum())} elements differ, first at {bad.nonzero()[0].tolist()}'
    print(f'{cid} exact: equal')
    d = fc_data(cid, 'bound')
    got = launch_fc(c, d)
    hold_to_bound(cid, got, d.ref, fc_bound(c, d))
    assert torch.equal(launch_fc(c, d), got), f'{cid}: two launches differ'


FC_M64 = [c for c in FC if c.M == 64]


@gpu
@pytest.mark.parametrize('cid', [c.id for c in FC_M64])
def test_fc_rows_alone_and_staging_give_the_same_bits(cid):
    c, d = FC_BY_ID[cid], fc_data(cid, 'bound')
    got = launch_fc(c, d)
    for m in (1, 32, 33):                                              # the last m rows: other rows of the tile, the other MT
        assert torch.equal(launch_fc(c, d, rows=slice(64 - m, 64)), got[64 - m:]), f'{cid}: {m} rows alone differ from M = 64'
    if c.K % 4 == 0:
        for off in (0, 1, 2, 3):                                       # vec at 0, scalar at 1 - 3
            assert torch.equal(launch_fc(c, d, off=off), got), f'{cid}: x misaligned by {off} floats differs'
    print(f'{cid} invariants: equal')


# ---------------------------------------------------------------------------------------------------------- refusals
def _set(**kw):
    def f(a):
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(a, k)[v[0]] = v[1]
            else:
                setattr(a, k, v)
    return f


FWD_REFUSED = {
    'Ci % 4': _set(Ci=6), 'wrong OH': _set(OH=4), 'wrong OW': _set(OW=4), 'Cop % bn': _set(bn=128), 'Cop < Co': _set(Cop=0),
    'bn = 32': _set(bn=32), 'nseg = 0': _set(nseg=0), 'nseg = 5': _set(nseg=5), 'seg_start[0] != 0': _set(seg_start=(0, 1)),
    'an unused slot below Co': _set(seg_start=(2, 32)), 'c0 + ncols > ldc': _set(ldc=(1, 13)), 'c0 < 0': _set(c0=(1, -1)),
    'an empty segment': _set(seg_start=(1, 0)), 'dst = NULL': _set(dst=(1, None)), 'SH = 0': _set(SH=0), 'KW = 0': _set(KW=0),
    'PH < 0': _set(PH=-1), 'N < 0': _set(N=-1), 'Co = 0': _set(Co=0), 'IH = 0': _set(IH=0),
}
BWD_REFUSED = {
    'a 1 x 1 kernel': _set(KH=1, KW=1, PH=0, PW=0), 'ldc != Co': _set(ldc=(0, 40)), 'c0 != 0': _set(c0=(0, 1)), 'nseg = 2': _set(nseg=2),
    'stride 2': _set(SH=2, SW=2, OH=2, OW=3), 'OH != IH': _set(OH=4), 'Ci % 4': _set(Ci=6), 'Cop % bn': _set(bn=128),
    'a used slot beyond the first': _set(seg_start=(1, 20)), 'dst = NULL': _set(dst=(0, None)), 'seg_start[0] != 0': _set(seg_start=(0, 1)),
    'Cop < Co': _set(Cop=0), 'pad 0': _set(PH=0, PW=0, OH=1, OW=3),
}
LIN_REFUSED = {
    'two segments': _set(nseg=2, seg_start=(1, 20)), 'c0 + Co > ldc': _set(ldc=(0, 37)), 'Ci % 4': _set(Ci=6), 'wrong OH': _set(OH=4),
    'Cop % bn': _set(bn=128), 'c0 < 0': _set(c0=(0, -1)), 'a used slot beyond the first': _set(seg_start=(3, 32)), 'dst = NULL': _set(dst=(0, None)),
    'seg_start[0] != 0': _set(seg_start=(0, 1)), 'nseg = 0': _set(nseg=0), 'KH = 0': _set(KH=0), 'Cop < Co': _set(Cop=0),
}


@gpu
def test_refused_calls_return_22_and_write_nothing():
    """One refused call per clause of the three validators and of fc_shape_ok; N = 0 returns 0 and writes nothing."""
    from rick_amd import gemm_conv
    from rick_amd._lib import lib
    n, h, w, ci, co = 2, 3, 5, 4, 33                                    # 3 x 3 stride 1 pad 1, Cop = bn = 64
    M = n * h * w
    fx, fw, fb, fr = Fenced(M * ci + 4), Fenced(64 * 64 + 4), Fenced(64), Fenced(M * 40)
    for f in (fx, fw, fb, fr):
        f.v.fill_(1.0)
    d0, d1 = Guarded(M * 40), Guarded(M * 14)

    def desc(kind, mutate=None, images=n):
        segs = {'fwd': [(p(d0), 40, 2, 20), (p(d1), 14, 1, 13)], 'bwd': [(p(d0), co, 0, co)], 'lin': [(p(d0), 40, 5, co)]}[kind]
        a = gemm_conv.descriptor(images, h, w, ci, (3, 3), (1, 1), (1, 1), 64, 64, segs)
        if mutate:
            mutate(a)
        return a

    def call(kind, a, xin=None, wpk=None, bias='', act=0):
        xin, wpk, bias = p(fx) if xin is None else xin, p(fw) if wpk is None else wpk, p(fb) if bias == '' else bias
        if kind == 'fwd':
            return lib.rick_inc_conv_f32(xin, wpk, bias, a, stream())
        if kind == 'bwd':
            return lib.rick_inc_conv_bwd_f32(xin, wpk, p(fr), p(fr), a, stream())
        return lib.rick_inc_conv_lin_f32(xin, wpk, bias, p(fr), act, a, stream())

    def refused(what, rc):
        torch.cuda.synchronize()
        assert rc == EINVAL, f'{what}: status {rc}'
        assert d0.untouched() and d1.untouched(), f'{what}: a refused call wrote'

    for kind, table in (('fwd', FWD_REFUSED), ('bwd', BWD_REFUSED), ('lin', LIN_REFUSED)):
        for what, mutate in table.items():
            refused(f'{kind}: {what}', call(kind, desc(kind, mutate)))
        refused(f'{kind}: misaligned in', call(kind, desc(kind), xin=p(fx) + 4))
        refused(f'{kind}: misaligned wpk', call(kind, desc(kind), wpk=p(fw) + 4))
        refused(f'{kind}: in = NULL', call(kind, desc(kind), xin=0))
        refused(f'{kind}: wpk = NULL', call(kind, desc(kind), wpk=0))
        refused(f'{kind}: no descriptor', call(kind, None))
        if kind != 'bwd':
            refused(f'{kind}: bias = NULL', call(kind, desc(kind), bias=None))
        rc = call(kind, desc(kind, images=0))
        torch.cuda.synchronize()
        assert rc == 0 and d0.untouched() and d1.untouched(), f'{kind}: N = 0 must return 0 and write nothing'
    refused('lin: act = 2', call('lin', desc('lin'), act=2))
    refused('lin: act = -1', call('lin', desc('lin'), act=-1))
    print(f'conv refusals: {len(FWD_REFUSED) + len(BWD_REFUSED) + len(LIN_REFUSED) + 19} calls returned 22 and wrote nothing; N = 0 returned 0')

    K, N = 8, 8
    x, wpk, b = Fenced(64 * K + 4), Fenced(lib.rick_fc_packed_floats(K, N) + 4), Fenced(N)
    ws, out = Guarded(65 * N), Guarded(65 * N)
    fc = lambda M=1, K=K, N=N, xp=p(x), wp=p(wpk), bp=p(b), wsp=p(ws), op=p(out): lib.rick_fc_f32(xp, wp, bp, wsp, op, M, K, N, 0, stream())
    calls = {'M = 65': fc(M=65), 'M = 0': fc(M=0), 'K = 0': fc(K=0), 'N = 0': fc(N=0), 'K > 2**24': fc(K=(1 << 24) + 1),
             'N > 2**20': fc(N=(1 << 20) + 1), 'misaligned wpk': fc(wp=p(wpk) + 4), 'x = NULL': fc(xp=None), 'wpk = NULL': fc(wp=None),
             'bias = NULL': fc(bp=None), 'ws = NULL': fc(wsp=None), 'out = NULL': fc(op=None)}
    torch.cuda.synchronize()
    for what, rc in calls.items():
        assert rc == EINVAL, f'fc: {what}: status {rc}'
    assert ws.untouched() and out.untouched(), 'fc: a refused call wrote'
    print(f'fc refusals: {len(calls)} calls returned 22 and wrote nothing')
