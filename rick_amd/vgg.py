"""VGG16 fc2 features on HIP kernels: the network behind the reference's improved precision / recall
(gan_metrics/precision_recall.py:124-152, ``IPR.extract_features``, as called from gan_training/eval.py:58-65).

    net = VGG16Fc2Features.load(src, device='cuda', batch=25)
    f = net(x)                                 # x [N, 3, H, W] fp32 in [-1, 1] -> [N, 4096] fp32 on x's device
    ev = Evaluator(g_ema, inception, real_feats, pr_feature_fn=net, real_pr_feats=net(real_images))

What the reference computes, step by step:

1. the images as the generator emits them, fp32 in [-1, 1]: no ImageNet affine on this path;
2. if H or W is not 224, ``F.interpolate(size=(224, 224))`` in its default mode 'nearest': source index
   ``min(int(floorf(dst * (float(in) / float(out)))), in - 1)`` with the scale held in fp32;
3. torchvision's ``vgg16().features``: 13 3x3 convolutions + ReLU and five 2x2 max pools -> [N, 512, 7, 7] (``avgpool`` is
   skipped);
4. ``.view(-1, 7 * 7 * 512)``: channel-major (c, y, x) order;
5. ``classifier[:4]`` = Linear(25088, 4096), ReLU, Dropout (identity in eval), Linear(4096, 4096): the feature is the fc2
   output before its ReLU.

CUDA fp32 inputs run rick_vgg_input_f32, the trunk shared with LPIPS (rick_amd/vgg_trunk.py: rick_inc_conv_f32 and
rick_lpips_maxpool2_f32, which also serves as the fifth pool) and rick_fc_f32 for the two linear layers (f32-input MFMA,
split-K partials summed in slice order; rick_amd/csrc/vgg.hip).  The trunk's activations are NHWC, so fc1's K axis is
permuted from (c, y, x) to (y, x, c) once at load time and the flatten is free.  An image's features are bit-identical
whatever batch it is computed in.  The workspace (input, the trunk's ping-pong buffers, one stage output, the fc hidden layer
and split-K partials for ``batch`` images) is allocated once in ``load``.  CPU tensors run the same network as a plain fp32
torch composition.

``src`` is a path to (or the contents of) a torchvision ``vgg16`` state_dict: ``features.{0,2,5,...,28}.{weight,bias}``,
``classifier.{0,3}.{weight,bias}``; ``classifier.6.*`` is accepted and ignored.
"""
import functools

import torch
import torch.nn.functional as F

from .fc import FC_MAX_ROWS, check_packed, pack_fc_weight, run_fc
from .netutil import check_images, cuda_device, get, load_dict
from .vgg_trunk import STAGES, VggTrunk, cpu_stages

SIZE = 224
POOLED = (7, 7, 512)            # (y, x, c) of the trunk's NHWC output after the fifth pool
FC_IN, FEATURES = 7 * 7 * 512, 4096


# ---- loading --------------------------------------------------------------------------------------------------------------
_get = functools.partial(get, who='VGG16Fc2Features', errors=(RuntimeError, RuntimeError))


def params_from_vgg16(sd):
    """torchvision vgg16 state_dict -> (convs {idx: (w, b)}, fcs [(w1 [4096, 25088], b1), (w2 [4096, 4096], b2)]) fp32 on
    the CPU, in torchvision's own layout."""
    used, convs = set(), {}
    for stage in STAGES:
        for idx, ci, co in stage:
            pre = f'features.{idx}'
            convs[idx] = (_get(sd, f'{pre}.weight', (co, ci, 3, 3)), _get(sd, f'{pre}.bias', (co,)))
            used |= {f'{pre}.weight', f'{pre}.bias'}
    fcs = []
    for idx, k in ((0, FC_IN), (3, FEATURES)):
        pre = f'classifier.{idx}'
        fcs.append((_get(sd, f'{pre}.weight', (FEATURES, k)), _get(sd, f'{pre}.bias', (FEATURES,))))
        used |= {f'{pre}.weight', f'{pre}.bias'}
    extra = sorted(k for k in sd if k not in used and not k.startswith('classifier.6.'))
    if extra:
        raise RuntimeError(f'VGG16Fc2Features: unexpected key {extra[0]!r} in the vgg16 state_dict')
    return convs, fcs


def permute_fc1(w):
    """fc1 weight [4096, 25088] with K in the reference's (c, y, x) flatten order -> K in the trunk's NHWC (y, x, c) order."""
    y, x, c = POOLED
    return w.view(w.shape[0], c, y, x).permute(0, 2, 3, 1).reshape(w.shape[0], FC_IN).contiguous()


# ---- resize ---------------------------------------------------------------------------------------------------------------
def nearest_index(n_in, n_out=SIZE):
    """Source index of every destination index of F.interpolate's 'nearest' mode, [n_out] int64: the product and the scale
    float(n_in) / float(n_out) are fp32, as in ATen."""
    scale = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    return (torch.arange(n_out, dtype=torch.float32) * scale).floor().to(torch.int64).clamp_(max=n_in - 1)


def resize_nearest(x):
    """x [N, C, H, W] -> [N, C, 224, 224] by the index rule (values copied); x itself at 224 x 224."""
    h, w = x.shape[2:]
    if (h, w) == (SIZE, SIZE):
        return x
    iy, ix = nearest_index(h).to(x.device), nearest_index(w).to(x.device)
    return x[:, :, iy][:, :, :, ix]


# ---- device plan ----------------------------------------------------------------------------------------------------------
class _Plan:
    """Workspace of `batch` images and the packed weights (device).

    Footprint: 164 floats per 224^2 pixel (the NHWC4 input 4, the trunk's ping-pong buffers 64 + 32, and `stage`, the
    destination of each stage's last convolution, 64) = 33 MB per image of `batch`, 0.8 GB at the default 25, next to 0.54 GB
    of packed weights (fc1 alone 411 MB).  Size `batch` with that in mind when the network sits beside a generator."""

    def __init__(self, convs, fcs, batch, device):
        from . import _lib
        self._lib = _lib
        lib = _lib.lib
        self.batch, self.pixels = batch, batch * SIZE * SIZE
        f32 = dict(device=device, dtype=torch.float32)
        self.trunk = VggTrunk(convs, device)
        self.x0 = torch.empty(self.pixels * 4, **f32)
        self.bufs = self.trunk.new_buffers(self.pixels, device)
        self.stage = torch.empty(self.pixels * 64, **f32)         # a stage's output; the first (64 channels at 224^2) is the largest
        rows = min(batch, FC_MAX_ROWS)
        self.fc, ws = [], 0
        for (w, b), relu in zip(fcs, (1, 0)):
            n, k = w.shape
            wpk = pack_fc_weight(permute_fc1(w) if k == FC_IN else w)
            check_packed(wpk, k, n, 'VGG16Fc2Features')
            self.fc.append((wpk.to(device), b.to(device), k, n, relu))
            ws = max(ws, lib.rick_fc_workspace_floats(rows, k, n))
        self.hidden = torch.empty(batch * FEATURES, **f32)
        self.ws = torch.empty(ws, **f32)

    def _fc(self, layer, src, rows, dst):
        wpk, b, k, n, relu = self.fc[layer]
        run_fc(src, wpk.data_ptr(), b.data_ptr(), self.ws.data_ptr(), dst, rows, k, n, relu)

    def run(self, x, out):
        """x [n, 3, H, W] fp32 contiguous, n <= batch -> out [n, 4096] (contiguous rows)."""
        lib = self._lib
        n, _, H, W = x.shape
        stream = lib.stream_ptr()
        lib.check(lib.lib.rick_vgg_input_f32(x.data_ptr(), self.x0.data_ptr(), n, H, W, stream), 'rick_vgg_input_f32')
        cur, h, w = self.trunk.run(self.x0.data_ptr(), n, SIZE, SIZE, self.bufs, lambda s: self.stage.data_ptr())
        lib.check(lib.lib.rick_lpips_maxpool2_f32(cur, self.bufs[0].data_ptr(), n, h, w, POOLED[2], stream),
                  'rick_lpips_maxpool2_f32')                      # the fifth pool: [n, 7, 7, 512] = [n, 25088] in (y, x, c) order
        self._fc(0, self.bufs[0].data_ptr(), n, self.hidden.data_ptr())
        self._fc(1, self.hidden.data_ptr(), n, out.data_ptr())


class VGG16Fc2Features:
    """torchvision vgg16 up to fc2 (before its ReLU) on HIP kernels; see the module docstring."""

    def __init__(self, convs, fcs, device='cuda', batch=25):
        if batch < 1:
            raise ValueError('VGG16Fc2Features: batch must be >= 1')
        self.convs, self.fcs = convs, fcs
        self.batch = int(batch)
        self.device = cuda_device(device)
        self._plan = None
        if self.device.type == 'cuda':
            with torch.cuda.device(self.device):
                self._plan = _Plan(convs, fcs, self.batch, self.device)

    @classmethod
    def load(cls, src, device='cuda', batch=25):
        """src: a path or state_dict in torchvision's vgg16 layout."""
        convs, fcs = params_from_vgg16(load_dict(src))
        return cls(convs, fcs, device=device, batch=batch)

    @torch.no_grad()
    def __call__(self, x):
        """x [N, 3, H, W] fp32 in [-1, 1] -> fc2 features [N, 4096] fp32 on x's device."""
        check_images(x, 'VGG16Fc2Features', self.device)
        N = x.shape[0]
        if x.device.type == 'cpu':
            out = torch.empty((N, FEATURES), dtype=torch.float32)
            (w1, b1), (w2, b2) = self.fcs
            for lo in range(0, N, self.batch):
                f = F.max_pool2d(cpu_stages(self.convs, resize_nearest(x[lo:lo + self.batch]))[-1], 2, 2)
                out[lo:lo + self.batch] = F.linear(F.relu(F.linear(f.reshape(f.shape[0], FC_IN), w1, b1)), w2, b2)
            return out
        out = torch.empty((N, FEATURES), device=x.device, dtype=torch.float32)
        x = x.contiguous()
        with torch.cuda.device(self.device):
            for lo in range(0, N, self.batch):
                hi = min(N, lo + self.batch)
                self._plan.run(x[lo:hi], out[lo:hi])
        return out
