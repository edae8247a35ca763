"""The VGG16 convolutional trunk (torchvision ``vgg16().features`` up to relu5_3) on HIP kernels, shared by LPIPS
(rick_amd/lpips.py: five taps) and the fc2 features behind precision / recall (rick_amd/vgg.py: the last stage only).

13 3x3 stride-1 pad-1 convolutions + ReLU on rick_inc_conv_f32 (f32-input MFMA, no split-K: an image's activations are
bit-identical whatever batch it is computed in), a 2x2 stride-2 max pool (rick_lpips_maxpool2_f32) in front of every stage
but the first.  Activations are NHWC fp32; the input is NHWC4 (channel 3 = 0)."""
import ctypes

import torch
import torch.nn.functional as F

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

    def __init__(self, convs, device):
        from . import _lib
        self._lib = _lib
        self.convs = []
        for stage in STAGES:
            for idx, ci, co in stage:
                w, b = convs[idx]
                cip = -(-ci // 4) * 4
                if cip != ci:                                       # the 3 input channels, padded to 4
                    w = F.pad(w, (0, 0, 0, 0, 0, cip - ci))
                K, bn = 9 * cip, 64 if co == 64 else 128
                Kp, Cop = -(-K // 32) * 32, -(-co // bn) * bn
                wpk = torch.zeros(Kp, Cop, dtype=torch.float32)
                wpk[:K, :co] = w.permute(2, 3, 1, 0).reshape(K, co)
                bp = torch.zeros(Cop, dtype=torch.float32)
                bp[:co] = b
                self.convs.append((cip, co, Cop, bn, wpk.to(device), bp.to(device)))

    def new_buffers(self, pixels, device):
        """The two ping-pong buffers for `pixels` level-0 pixels."""
        need = pingpong_need()
        f32 = dict(device=device, dtype=torch.float32)
        return [torch.empty(int(pixels * need[0]), **f32), torch.empty(max(1, int(pixels * need[1])), **f32)]

    def _conv(self, k, src, n, h, w, dst):
        lib = self._lib
        ci, co, cop, bn, wpk, bp = self.convs[k]
        a = lib.IncConv()
        a.N, a.IH, a.IW, a.Ci, a.KH, a.KW, a.SH, a.SW, a.PH, a.PW, a.OH, a.OW = n, h, w, ci, 3, 3, 1, 1, 1, 1, h, w
        a.Co, a.Cop, a.bn, a.nseg = co, cop, bn, 1
        for i in range(4):
            a.seg_start[i], a.ldc[i], a.c0[i], a.dst[i] = (0, co, 0, dst) if i == 0 else (co, 0, 0, None)
        lib.check(lib.lib.rick_inc_conv_f32(src, wpk.data_ptr(), bp.data_ptr(), ctypes.byref(a), lib.stream_ptr()),
                  'rick_inc_conv_f32')

    def run(self, src, n, h, w, bufs, stage_dst, after_stage=None):
        """src: pointer to the NHWC4 input [n, h, w, 4].  Stage s's last convolution writes to the pointer stage_dst(s)
        ([n, h_s, w_s, C_s]; it must not alias bufs); after_stage(s, ptr, n, h_s, w_s), if given, is called once that
        convolution is enqueued.  Returns (pointer, h, w) of the last stage's output."""
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
                dst = stage_dst(s) if j == len(stage) - 1 else bufs[flip].data_ptr()
                self._conv(k, cur, n, h, w, dst)
                cur, flip, k = dst, 1 - flip, k + 1
            if after_stage is not None:
                after_stage(s, cur, n, h, w)
        return cur, h, w
