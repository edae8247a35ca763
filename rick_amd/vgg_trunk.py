"""The VGG16 convolutional trunk (torchvision ``vgg16().features`` up to relu5_3) on HIP kernels, shared by LPIPS
(rick_amd/lpips.py: five taps) and the fc2 features behind precision / recall (rick_amd/vgg.py: the last stage only).

13 3x3 stride-1 pad-1 convolutions + ReLU on rick_inc_conv_f32 (f32-input MFMA, no split-K: an image's activations are
bit-identical whatever batch it is computed in), a 2x2 stride-2 max pool (rick_lpips_maxpool2_f32) in front of every stage
but the first.  Activations are NHWC fp32; the input is NHWC4 (channel 3 = 0).

With ``transposed=True`` the trunk also holds every filter packed transposed and rotated, and ``run_backward`` carries a
gradient from the five stage outputs back to the NHWC4 input on rick_inc_conv_bwd_f32 and rick_lpips_maxpool2_bwd_f32 (data
gradients only: the weights are constants).  The GEMM operands, descriptors and launches are rick_amd/gemm_conv.py's."""
import torch
import torch.nn.functional as F

from . import gemm_conv
from .gemm_conv import pack_transposed  # noqa: F401  (part of this module's surface)

K3 = ((3, 3), (1, 1), (1, 1))           # kernel, stride, padding of every convolution

# (features index, Ci, Co) of the 13 convolutions, grouped by stage; a 2x2 max pool precedes every stage but the first
STAGES = [[(0, 3, 64), (2, 64, 64)], [(5, 64, 128), (7, 128, 128)], [(10, 128, 256), (12, 256, 256), (14, 256, 256)],
          [(17, 256, 512), (19, 512, 512), (21, 512, 512)], [(24, 512, 512), (26, 512, 512), (28, 512, 512)]]
CHANNELS = (64, 128, 256, 512, 512)


def cpu_stages(convs, x):
    """fp32 torch composition: x [N, 3, H, W] -> the five stage outputs (relu1_2 ... relu5_3), NCHW."""
    outs = []
    for s, stage in enumerate(STAGES):
        if s:
            x = F.max_pool2d(x, 2, 2)
        for idx, _, _ in stage:
            w, b = convs[idx]
            x = F.relu(F.conv2d(x, w, b, 1, 1))
        outs.append(x)
    return outs


def pingpong_need():
    """Capacity of the two ping-pong buffers in floats per level-0 pixel: walk the stages (buffer 0 <- pool / first conv,
    alternate within a stage; a stage's last convolution writes its own destination)."""
    need, area = [0.0, 0.0], 1.0
    for s, stage in enumerate(STAGES):
        if s:
            area /= 4
            need[0] = max(need[0], area * stage[0][1])          # pool output
            cur = 0
        else:
            cur = None
        for k, (_, _, co) in enumerate(stage[:-1]):
            dst = 0 if cur is None else 1 - cur
            need[dst] = max(need[dst], area * co)
            cur = dst
    return need


class VggTrunk:
    """The packed convolution weights (device) and the launch sequence of the trunk."""

    def __init__(self, convs, device, transposed=False):
        from . import _lib
        self._lib = _lib
        self.convs = []
        self.convs_t = []            # (Ci of the gradient GEMM, Co, Cop, bn, wt) per convolution, with `transposed`
        for stage in STAGES:
            for idx, ci, co in stage:
                w, b = convs[idx]
                cip = -(-ci // 4) * 4                               # the 3 input channels, padded to 4
                wpk, bp, cop, bn = gemm_conv.pack(w, b, ci_pad=cip)
                self.convs.append((cip, co, cop, bn, wpk.to(device), bp.to(device)))
                if transposed:
                    wt, cop_t, bn_t = pack_transposed(w, ci_pad=cip)
                    self.convs_t.append((co, cip, cop_t, bn_t, wt.to(device)))

    def new_buffers(self, pixels, device):
        """The two ping-pong buffers for `pixels` level-0 pixels."""
        need = pingpong_need()
        f32 = dict(device=device, dtype=torch.float32)
        return [torch.empty(int(pixels * need[0]), **f32), torch.empty(max(1, int(pixels * need[1])), **f32)]

    def _conv(self, k, src, n, h, w, dst):
        ci, co, cop, bn, wpk, bp = self.convs[k]
        gemm_conv.forward(src, wpk.data_ptr(), bp.data_ptr(), gemm_conv.descriptor(n, h, w, ci, *K3, cop, bn, [(dst, co, 0, co)]))

    def run(self, src, n, h, w, bufs, stage_dst, after_stage=None, keep=None):
        """src: pointer to the NHWC4 input [n, h, w, 4].  Stage s's last convolution writes to the pointer stage_dst(s)
        ([n, h_s, w_s, C_s]; it must not alias bufs); after_stage(s, ptr, n, h_s, w_s), if given, is called once that
        convolution is enqueued.  keep, if given, holds 13 pointers: convolution k that does not end a stage writes keep[k]
        rather than a ping-pong buffer (the activations run_backward needs).  Returns (pointer, h, w) of the last stage's
        output."""
        lib = self._lib
        stream = lib.stream_ptr()
        cur, k = src, 0
        for s, stage in enumerate(STAGES):
            if s:
                c = CHANNELS[s - 1]
                lib.check(lib.lib.rick_lpips_maxpool2_f32(cur, bufs[0].data_ptr(), n, h, w, c, stream),
                          'rick_lpips_maxpool2_f32')
                cur, h, w, flip = bufs[0].data_ptr(), h // 2, w // 2, 1
            else:
                flip = 0
            for j in range(len(stage)):
                dst = stage_dst(s) if j == len(stage) - 1 else bufs[flip].data_ptr() if keep is None else keep[k]
                self._conv(k, cur, n, h, w, dst)
                cur, flip, k = dst, 1 - flip, k + 1
            if after_stage is not None:
                after_stage(s, cur, n, h, w)
        return cur, h, w

    def _conv_bwd(self, k, gout, n, h, w, mask, dst):
        ci, co, cop, bn, wt = self.convs_t[k]
        gemm_conv.backward(gout, wt.data_ptr(), mask, None, gemm_conv.descriptor(n, h, w, ci, *K3, cop, bn, [(dst, co, 0, co)]))

    def run_backward(self, n, h, w, acts, gbufs, tap_grad):
        """The mirror of run: acts holds the pointers of the 13 stored activations of n images of h x w (a stage's last entry
        is its output), gbufs three buffers of n * h * w * 64 floats.  tap_grad(s, ptr, n, h_s, w_s, relu) enqueues the
        gradient that reaches stage s's output from outside into ptr [n, h_s, w_s, C_s]: through that output's ReLU for the
        last stage (relu = True), as it stands for the others, whose ReLU the pool adjoint applies.  Returns the pointer (one
        of gbufs) of the gradient with respect to the NHWC4 input [n, h, w, 4]."""
        lib = self._lib
        stream = lib.stream_ptr()
        dims = [(h >> s, w >> s) for s in range(len(STAGES))]
        k = sum(len(stage) for stage in STAGES) - 1
        hs, ws = dims[-1]
        cur, flip = gbufs[0].data_ptr(), 1
        tap_grad(len(STAGES) - 1, cur, n, hs, ws, True)
        for s in range(len(STAGES) - 1, -1, -1):
            hs, ws = dims[s]
            for j in range(len(STAGES[s]) - 1, -1, -1):
                dst = gbufs[flip].data_ptr()
                self._conv_bwd(k, cur, n, hs, ws, acts[k - 1] if j else None, dst)
                cur, flip, k = dst, 1 - flip, k - 1
            if s:
                hs, ws = dims[s - 1]
                tap_grad(s - 1, gbufs[2].data_ptr(), n, hs, ws, False)
                dst = gbufs[flip].data_ptr()
                lib.check(lib.lib.rick_lpips_maxpool2_bwd_f32(acts[k], gbufs[2].data_ptr(), cur, dst, n, hs, ws, CHANNELS[s - 1],
                                                              stream), 'rick_lpips_maxpool2_bwd_f32')
                cur, flip = dst, 1 - flip
        return cur
