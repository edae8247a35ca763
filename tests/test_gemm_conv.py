"""CPU: the host side of the f32 GEMM convolution (rick_amd/gemm_conv.py) against an independent restatement of the operand
layout of rick_inc_conv_f32 / rick_inc_conv_bwd_f32 (include/rick_hip.h), on every convolution the project runs: the 94
Inception units, the fused head groups the Inception plan launches, the 13 VGG convolutions in both directions and the shapes
of the GPU gradient test.  The column blocks are held to a literal table, the descriptor to hand-written fields."""
import pytest
import torch
import torch.nn.functional as F

from rick_amd import gemm_conv
from rick_amd.inception import units
from rick_amd.vgg_trunk import STAGES

# Co -> (bn, Cop): what the three rules this module's one rule replaced gave on every layer (single units, fused groups, VGG)
UNIT_BLOCKS = {32: (64, 64), 48: (64, 64), 64: (64, 64), 80: (128, 128), 96: (128, 128), 128: (128, 128), 160: (64, 192),
               192: (64, 192), 320: (64, 320), 384: (128, 384), 448: (64, 448)}
# fused 1x1 heads: A 64 + 48 + 64, C 192 + 2 c7 (c7 = 128, 160, 192), D 192 + 192, E 320 + 384 + 448
GROUP_BLOCKS = {176: (64, 192), 448: (64, 448), 512: (128, 512), 576: (64, 576), 384: (128, 384), 1152: (128, 1152)}
VGG_BLOCKS = {64: (64, 64), 128: (128, 128), 256: (128, 256), 512: (128, 512)}
VGG_T_BLOCKS = {4: (64, 64), 64: (64, 64), 128: (128, 128), 256: (128, 256), 512: (128, 512)}


def restated(w, bn):
    """[Kp, Cop] from w [Co, Ci, kh, kw] by index arithmetic on the flat weight: row r = (ky kw + kx) Ci + ci, column co."""
    co, ci, kh, kw = w.shape
    K = kh * kw * ci
    Kp, cop = (K + 31) // 32 * 32, (co + bn - 1) // bn * bn
    r, c = torch.arange(Kp)[:, None], torch.arange(cop)[None, :]
    ky, kx, cin = r // (kw * ci), r // ci % kw, r % ci
    live = (r < K) & (c < co)
    flat = ((c * ci + cin) * kh + ky) * kw + kx
    return torch.where(live, w.reshape(-1)[torch.where(live, flat, torch.zeros_like(flat))], torch.zeros(()))


def rotated(w):
    """[Ci, Co, kh, kw]: the filter of the data gradient, element by element."""
    co, ci, kh, kw = w.shape
    out = torch.empty(ci, co, kh, kw)
    for ky in range(kh):
        for kx in range(kw):
            out[:, :, ky, kx] = w[:, :, kh - 1 - ky, kw - 1 - kx].t()
    return out


def check_pair(w, b, want, want_t=None, ci_pad=None):
    """The forward operand of (w, b) and the transposed operand of w against the restatement; want = (bn, Cop)."""
    wpk, bp, cop, bn = gemm_conv.pack(w, b, ci_pad=ci_pad)
    wp = w if ci_pad is None else F.pad(w, (0, 0, 0, 0, 0, ci_pad - w.shape[1]))
    co = w.shape[0]
    assert (bn, cop) == want and bn == gemm_conv.column_block(co)
    assert wpk.dtype == bp.dtype == torch.float32 and wpk.device.type == 'cpu'
    assert torch.equal(wpk, restated(wp, bn))
    assert torch.equal(bp[:co], b) and bp.shape == (cop,) and torch.all(bp[co:] == 0)
    wt, cop_t, bn_t = gemm_conv.pack_transposed(w, ci_pad=ci_pad)
    if want_t is not None:
        assert (bn_t, cop_t) == want_t
    assert bn_t == gemm_conv.column_block(wp.shape[1]) and cop_t % bn_t == 0 and 0 <= cop_t - wp.shape[1] < bn_t
    assert torch.equal(wt, restated(rotated(wp), bn_t))


def rand_conv(g, co, ci, kh, kw):
    return torch.randn(co, ci, kh, kw, generator=g), torch.randn(co, generator=g)


def test_small_case_by_loops():
    """Every element of a small operand, its padding included, by loops over (ky, kx, ci, co)."""
    g = torch.Generator().manual_seed(0)
    w, b = rand_conv(g, 5, 3, 2, 3)
    for bn in (None, 64, 128):
        wpk, bp, cop, got_bn = gemm_conv.pack(w, b, ci_pad=4, bn=bn)
        assert (got_bn, cop) == ((64, 64) if bn is None else (bn, bn)) and wpk.shape == (32, cop)
        want = torch.zeros(32, cop)
        for ky in range(2):
            for kx in range(3):
                for ci in range(3):
                    for co in range(5):
                        want[(ky * 3 + kx) * 4 + ci, co] = w[co, ci, ky, kx]
        assert torch.equal(wpk, want) and torch.equal(bp, F.pad(b, (0, cop - 5)))
    wt, cop, bn = gemm_conv.pack_transposed(w, ci_pad=4)
    want = torch.zeros(32, 64)
    for ky in range(2):
        for kx in range(3):
            for ci in range(3):
                for co in range(5):
                    want[(ky * 3 + kx) * 5 + co, ci] = w[co, ci, 1 - ky, 2 - kx]
    assert (cop, bn) == (64, 64) and torch.equal(wt, want)
    assert torch.equal(gemm_conv.pack(w)[1], torch.zeros(64))             # no bias: zeros
    assert gemm_conv.column_block(130) == 64 and gemm_conv.column_block(129) == 64 and gemm_conv.column_block(257) == 64


def test_every_inception_unit():
    g = torch.Generator().manual_seed(1)
    us = units(3)
    assert len(us) == 94 and {u[2] for u in us} == set(UNIT_BLOCKS)
    for name, ci, co, (kh, kw), _, _ in us:
        w, b = rand_conv(g, co, ci, kh, kw)
        check_pair(w, b, UNIT_BLOCKS[co], ci_pad=4 if ci == 3 else None)


def test_every_fused_head_group_of_the_plan():
    """The groups are read off the plan itself: its dry walk, with the convolution step replaced by a recorder."""
    from rick_amd import inception as inc
    rec = []

    class Recorder(inc._Plan):
        def _conv(self, us, P, src, h, w, ci, dsts):
            rec.append((us, ci))

    Recorder({}, 3, 1, 'cpu')
    half = len(rec) // 2                                                   # the walk runs twice
    assert rec[:half] == rec[half:] and sum(len(us) for us, _ in rec[:half]) == 94
    groups = [(us, ci) for us, ci in rec[:half] if len(us) > 1]
    kinds = [len(us) for us, _ in groups]
    assert kinds == [3] * 3 + [3] * 4 + [2] + [3] * 2                      # A x 3, C x 4, D, E x 2
    assert {sum(u[2] for u in us) for us, _ in groups} == set(GROUP_BLOCKS)
    g = torch.Generator().manual_seed(2)
    for us, ci in groups:
        ws, bs = zip(*[rand_conv(g, u[2], ci, 1, 1) for u in us])
        check_pair(torch.cat(ws), torch.cat(bs), GROUP_BLOCKS[sum(u[2] for u in us)])


def test_every_vgg_convolution_both_directions():
    g = torch.Generator().manual_seed(3)
    for stage in STAGES:
        for _, ci, co in stage:
            w, b = rand_conv(g, co, ci, 3, 3)
            cip = -(-ci // 4) * 4
            check_pair(w, b, VGG_BLOCKS[co], VGG_T_BLOCKS[cip], ci_pad=cip)


@pytest.mark.parametrize('ci,co', [(64, 3), (64, 64), (128, 64), (512, 256)])
def test_gradient_test_shapes(ci, co):
    """tests/test_gpu_lpips_grad.py: the gradient GEMM with ci input channels and co (padded to 4) columns."""
    from rick_amd.vgg_trunk import pack_transposed
    assert pack_transposed is gemm_conv.pack_transposed
    wf = torch.randn(ci, co, 3, 3, generator=torch.Generator().manual_seed(ci + co))
    cols = -(-co // 4) * 4
    wt, cop, bn = pack_transposed(F.pad(wf, (0, 0, 0, 0, 0, cols - co)))
    assert (bn, cop) == VGG_T_BLOCKS[cols] and wt.shape == ((9 * ci + 31) // 32 * 32, cop)
    assert torch.equal(wt, restated(rotated(F.pad(wf, (0, 0, 0, 0, 0, cols - co))), bn))


def fields(a):
    return dict(scalars=[getattr(a, n) for n in ('N', 'IH', 'IW', 'Ci', 'KH', 'KW', 'SH', 'SW', 'PH', 'PW', 'OH', 'OW', 'Co', 'Cop',
                                                 'bn', 'nseg')],
                seg_start=list(a.seg_start), ldc=list(a.ldc), c0=list(a.c0), dst=list(a.dst))


def test_descriptor_fields():
    from rick_amd._lib import IncConv
    # InceptionA's three fused heads at 35 x 35 on 192 channels: into the block's output and two scratch buffers
    a = gemm_conv.descriptor(2, 35, 35, 192, (1, 1), (1, 1), (0, 0), 192, 64,
                             [(0x1000, 256, 32, 64), (0x2000, 48, 0, 48), (0x3000, 64, 0, 64)])
    assert isinstance(a, IncConv)
    assert fields(a) == dict(scalars=[2, 35, 35, 192, 1, 1, 1, 1, 0, 0, 35, 35, 176, 192, 64, 3], seg_start=[0, 64, 112, 176],
                             ldc=[256, 48, 64, 0], c0=[32, 0, 0, 0], dst=[0x1000, 0x2000, 0x3000, None])
    # one segment, forward: a strided, unpadded 3 x 3 on a 299 x 280 NHWC4 input
    a = gemm_conv.descriptor(3, 299, 280, 4, (3, 3), (2, 2), (0, 0), 64, 64, [(0x4000, 45, 5, 32)])
    assert fields(a) == dict(scalars=[3, 299, 280, 4, 3, 3, 2, 2, 0, 0, 149, 139, 32, 64, 64, 1], seg_start=[0, 32, 32, 32],
                             ldc=[45, 0, 0, 0], c0=[5, 0, 0, 0], dst=[0x4000, None, None, None])
    # backward: the gradient of the first VGG convolution, 64 channels in, the image's 4 out
    a = gemm_conv.descriptor(3, 9, 5, 64, (3, 3), (1, 1), (1, 1), 64, 64, [(0x5000, 4, 0, 4)])
    assert fields(a) == dict(scalars=[3, 9, 5, 64, 3, 3, 1, 1, 1, 1, 9, 5, 4, 64, 64, 1], seg_start=[0, 4, 4, 4],
                             ldc=[4, 0, 0, 0], c0=[0, 0, 0, 0], dst=[0x5000, None, None, None])
    # asymmetric kernels keep the size under their own padding
    assert gemm_conv.out_hw(17, 17, (1, 7), (1, 1), (0, 3)) == (17, 17) and gemm_conv.out_hw(17, 17, (7, 1), (1, 1), (3, 0)) == (17, 17)
