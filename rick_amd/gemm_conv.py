"""The host side of rick_inc_conv_f32 / rick_inc_conv_bwd_f32 (include/rick_hip.h), the f32 implicit-GEMM convolution every
evaluation network runs on (rick_amd/inception.py, rick_amd/vgg_trunk.py): the GEMM operand, the choice of the column block,
the rick_inc_conv descriptor and the two launches.  The one definition of each; tests/test_gemm_conv.py restates the layout
independently.  The shared library is imported when a descriptor is built or a kernel launched, not before."""
import functools

import torch
import torch.nn.functional as F


@functools.cache
def _lib():
    from . import _lib
    return _lib


def out_hw(h, w, k, s, p):
    return (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1


def column_block(co):
    """The column block bn in {64, 128} that pads co columns least; 128 on a tie."""
    return 128 if -(-co // 128) * 128 == -(-co // 64) * 64 else 64


def _pad_ci(w, ci_pad):
    if ci_pad is not None and w.shape[1] < ci_pad:                # the image's 3 channels travel as 4
        w = F.pad(w, (0, 0, 0, 0, 0, ci_pad - w.shape[1]))
    return w


def pack(w, bias=None, ci_pad=None, bn=None):
    """w [Co, Ci, kh, kw] (Ci zero-padded to ci_pad) -> the forward GEMM operand wpk [Kp, Cop], wpk[(ky, kx, ci), co] =
    w[co, ci, ky, kx], K = kh kw Ci rounded up to 32 rows and Co to the column block bn (column_block(Co) unless given), and
    the bias [Cop], all padding zero.  Heads that share an input are concatenated along Co by the caller.  Returns fp32 CPU
    tensors and the block: (wpk, bias, Cop, bn)."""
    w = _pad_ci(w, ci_pad)
    co, ci, kh, kw = w.shape
    K, bn = kh * kw * ci, bn or column_block(co)
    Kp, cop = -(-K // 32) * 32, -(-co // bn) * bn
    wpk = torch.zeros(Kp, cop, dtype=torch.float32)
    wpk[:K, :co] = w.permute(2, 3, 1, 0).reshape(K, co)
    bp = torch.zeros(cop, dtype=torch.float32)
    if bias is not None:
        bp[:co] = bias
    return wpk, bp, cop, bn


def pack_transposed(w, ci_pad=None):
    """w [Co, Ci, kh, kw] -> the data gradient's GEMM operand: the forward operand of the rotated, transposed filter, rows
    (ky, kx, co), columns ci, Wt[(ky, kx, co)][ci] = W[co][ci][kh - 1 - ky][kw - 1 - kx].  Returns (wt, Cop, bn)."""
    wt, _, cop, bn = pack(_pad_ci(w, ci_pad).flip(2, 3).transpose(0, 1))
    return wt, cop, bn


def descriptor(n, h, w, ci, k, s, p, cop, bn, segs):
    """The rick_inc_conv of n images [h, w, ci] under a kernel k = (kh, kw), stride s and padding p, on an operand of cop
    columns in blocks of bn.  segs: up to four (dst pointer, ldc, c0, ncols): consecutive runs of ncols GEMM columns, each
    written to channels [c0, c0 + ncols) of a destination with ldc channels; Co is their sum.  Unused slots start at Co and
    keep the structure's zeros: (Co, 0, 0, None)."""
    co = sum([seg[3] for seg in segs])
    a = _lib().IncConv(n, h, w, ci, *k, *s, *p, *out_hw(h, w, k, s, p), co, cop, bn, len(segs))
    start = 0
    for i, (dst, ldc, c0, ncols) in enumerate(segs):
        a.seg_start[i], a.ldc[i], a.c0[i], a.dst[i] = start, ldc, c0, dst
        start += ncols
    for i in range(len(segs), 4):
        a.seg_start[i] = co
    return a


def forward(src, wpk, bias, a, stream=None):
    """relu(conv(src) + bias) into the descriptor's destinations (pointers; stream: the current one unless given)."""
    lib = _lib()
    lib.check(lib.lib.rick_inc_conv_f32(src, wpk, bias, a, lib.stream_ptr() if stream is None else stream), 'rick_inc_conv_f32')


def backward(gout, wt, mask, add, a):
    """The data gradient on a pack_transposed operand: (conv(gout) [+ add]) [where mask > 0], on the current stream."""
    lib = _lib()
    lib.check(lib.lib.rick_inc_conv_bwd_f32(gout, wt, mask, add, a, lib.stream_ptr()), 'rick_inc_conv_bwd_f32')
