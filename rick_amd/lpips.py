"""LPIPS with the VGG16 backbone on HIP kernels: the metric behind the reference's intra-cluster LPIPS (gan_training/eval.py,
which calls ``lpips.LPIPS(net='vgg')`` from richzhang/PerceptualSimilarity).

    net = LPIPS.load(src, device='cuda', batch=25)
    d = net(x, y)                              # x, y [N, 3, H, W] fp32 in [-1, 1] -> [N]
    fa, fb = net.features(xa), net.features(xb)
    D = net.distances(fa, fb)                  # [na, nb]

The definitions are those of lpips 0.1.x (``LPIPS(net='vgg')``, version '0.1', ``lpips=True``, ``spatial=False``) over
torchvision's ``vgg16().features``:

1. scaling layer ``(x - shift) / scale``, shift = (-.030, -.088, -.188), scale = (.458, .448, .450);
2. the VGG16 trunk up to relu5_3 (``features[0:30]``: 3x3 stride-1 pad-1 convolutions + ReLU, 2x2 stride-2 max pools with
   floor at indices 4, 9, 16, 23), tapped after indices 3, 8, 15, 22 and 29 (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3);
3. at every tap each position's channel vector divided by ``sqrt(sum_c f_c^2) + 1e-10``;
4. ``d_l = mean over (h, w) of sum_c w_lc (fx_hat - fy_hat)^2`` with the 1x1 "lin" weights w_l (no bias; dropout is off);
5. ``LPIPS = d_0 + ... + d_4``.

An image's taps do not depend on the image it is compared with, so ``features`` runs the trunk once per image and keeps the
five taps (NHWC) and their per-position inverse norms; ``distances`` then forms every pair of two feature sets with
rick_lpips_pair_f32 in the direct form ``sum_c w_c (a_c ia - b_c ib)^2`` (never the Gram form, which cancels on near pairs).

CUDA fp32 inputs run the kernels of rick_amd/csrc/lpips.hip and the Inception convolution rick_inc_conv_f32 (f32-input MFMA,
no split-K: an image's taps are bit-identical whatever batch it is computed in).  The workspace (input, two ping-pong
activation buffers and one tap set of ``batch`` images at ``size`` x ``size``) is allocated once in ``load``.  CPU tensors
run the same network as a plain fp32 torch composition.

``src`` is a path to (or the contents of) either ``lpips.LPIPS(net='vgg').state_dict()`` (``net.slice{1..5}.{idx}.*``,
``lin{k}.model.1.weight``, optionally the ``lins.{k}.*`` duplicates and the ``scaling_layer.*`` buffers), or use
``LPIPS.load(vgg=..., lin=...)`` with a torchvision ``vgg16`` state_dict (``features.{idx}.*``; ``classifier.*`` ignored)
and the lin weights file (``lin{k}.model.1.weight``, the layout of lpips' ``weights/v0.1/vgg.pth``).
"""
import ctypes

import torch

from .vgg_trunk import CHANNELS, STAGES, VggTrunk, cpu_stages

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
EPS = 1e-10
SIZE = 256
TAPS = (3, 8, 15, 22, 29)
SLICE_OF = {idx: s + 1 for s, stage in enumerate(STAGES) for idx, _, _ in stage}     # lpips' net.slice{1..5}
PAIR_SLICE_ELEMS = 8192      # feature elements per pair-kernel slice: positions per slice = 8192 // C, fixed per tap


def _tap_hw(h, w):
    out = []
    for s in range(5):
        if s:
            h, w = h // 2, w // 2
        out.append((h, w))
    return out


def _positions_per_slice(c):
    return max(1, PAIR_SLICE_ELEMS // c)


# ---- loading --------------------------------------------------------------------------------------------------------------
def _get(sd, key, shape):
    if key not in sd:
        raise KeyError(f'LPIPS: missing key {key!r}')
    v = torch.as_tensor(sd[key])
    if tuple(v.shape) != tuple(shape):
        raise ValueError(f'LPIPS: key {key!r} has shape {tuple(v.shape)}, expected {tuple(shape)}')
    return v.detach().to('cpu', torch.float32).contiguous()


def _check_scaling(sd, key, ref):
    v = _get(sd, key, (1, 3, 1, 1)).flatten()
    if not torch.equal(v, torch.tensor(ref, dtype=torch.float32)):
        raise ValueError(f'LPIPS: {key!r} = {v.tolist()} differs from lpips 0.1 {list(ref)}')


def _lin_weights(sd, used, prefix='lin'):
    lins = []
    for k, c in enumerate(CHANNELS):
        key = f'{prefix}{k}.model.1.weight'
        lins.append(_get(sd, key, (1, c, 1, 1)).flatten())
        used.add(key)
    return lins


def _unknown(sd, used, what):
    extra = sorted(k for k in sd if k not in used)
    if extra:
        raise KeyError(f'LPIPS: unexpected key {extra[0]!r} in the {what}')


def params_from_lpips(sd):
    """lpips.LPIPS(net='vgg').state_dict() layout -> (convs {idx: (w, b)}, lins [5 x [C]]) fp32 on the CPU."""
    used, convs = set(), {}
    for stage in STAGES:
        for idx, ci, co in stage:
            pre = f'net.slice{SLICE_OF[idx]}.{idx}'
            convs[idx] = (_get(sd, f'{pre}.weight', (co, ci, 3, 3)), _get(sd, f'{pre}.bias', (co,)))
            used |= {f'{pre}.weight', f'{pre}.bias'}
    lins = _lin_weights(sd, used)
    for k, c in enumerate(CHANNELS):              # the ModuleList duplicates, when present, must agree
        key = f'lins.{k}.model.1.weight'
        if key in sd:
            if not torch.equal(_get(sd, key, (1, c, 1, 1)).flatten(), lins[k]):
                raise ValueError(f'LPIPS: {key!r} differs from lin{k}.model.1.weight')
            used.add(key)
    for key, ref in (('scaling_layer.shift', SHIFT), ('scaling_layer.scale', SCALE)):
        if key in sd:
            _check_scaling(sd, key, ref)
            used.add(key)
    _unknown(sd, used, 'lpips state_dict')
    return convs, lins


def params_from_vgg(vgg, lin):
    """torchvision vgg16 state_dict (classifier.* ignored; features beyond relu5_3 are an error) + lin weights file."""
    used, convs = set(), {}
    for stage in STAGES:
        for idx, ci, co in stage:
            pre = f'features.{idx}'
            convs[idx] = (_get(vgg, f'{pre}.weight', (co, ci, 3, 3)), _get(vgg, f'{pre}.bias', (co,)))
            used |= {f'{pre}.weight', f'{pre}.bias'}
    used |= {k for k in vgg if k.startswith('classifier.')}
    _unknown(vgg, used, 'vgg16 state_dict')
    used_lin = set()
    lins = _lin_weights(lin, used_lin)
    _unknown(lin, used_lin, 'lin weights')
    return convs, lins


def _load_dict(src):
    if src is None or isinstance(src, dict):
        return src
    return torch.load(src, map_location='cpu', weights_only=True)


# ---- features -------------------------------------------------------------------------------------------------------------
class LpipsFeatures:
    """Taps [n, h_l, w_l, C_l] (NHWC fp32) and inverse norms [n, h_l * w_l] of n images, l = 0..4."""

    def __init__(self, taps, inorm):
        self.taps, self.inorm = taps, inorm

    @classmethod
    def empty(cls, n, h, w, device):
        kw = dict(device=device, dtype=torch.float32)
        hw = _tap_hw(h, w)
        return cls([torch.empty((n, a, b, c), **kw) for (a, b), c in zip(hw, CHANNELS)],
                   [torch.empty((n, a * b), **kw) for a, b in hw])

    @property
    def n(self):
        return self.taps[0].shape[0]

    @property
    def size(self):
        return tuple(self.taps[0].shape[1:3])

    @property
    def device(self):
        return self.taps[0].device

    def narrow(self, lo, hi):
        """Images [lo, hi) as views."""
        return LpipsFeatures([t[lo:hi] for t in self.taps], [t[lo:hi] for t in self.inorm])


def scale_input(x, quantize=False):
    """The input as lpips sees it, fp32 on x's device: uint8 x -> q / 255 -> (t - 0.5) / 0.5; float x with ``quantize``
    -> first q = uint8(clamp((x / 2 + 0.5) * 255 + 0.5, 0, 255)) (the reference's PNG files); then (x - shift) / scale.
    Returns (scaled [N, 3, H, W], q or None)."""
    q = None
    if x.dtype == torch.uint8:
        q = x
    elif quantize:
        q = ((x / 2 + 0.5) * 255 + 0.5).clamp(0, 255).to(torch.uint8)
    if q is not None:
        x = (q.to(torch.float32) / 255 - 0.5) / 0.5
    shift = torch.tensor(SHIFT, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    return (x - shift) / scale, q


_cpu_taps = cpu_stages            # the five taps are the five stage outputs of the shared trunk


def _inverse_norm(f, dim):
    s = (f * f).sum(dim)
    return torch.where(s > 0, 1.0 / (s.sqrt() + EPS), torch.zeros_like(s))


class _Plan:
    """Workspace of `batch` images at size x size and the shared trunk's packed convolution weights (device)."""

    def __init__(self, convs, lins, batch, size, device):
        from . import _lib
        self._lib = _lib
        self.batch, self.size, self.pixels = batch, size, batch * size * size
        self.trunk = VggTrunk(convs, device)
        self.x0 = torch.empty(self.pixels * 4, device=device, dtype=torch.float32)
        self.bufs = self.trunk.new_buffers(self.pixels, device)
        self.lins = [w.to(device) for w in lins]

    def run(self, x, mode, out, u8out):
        """x [n, 3, H, W] (fp32, or uint8 for mode 2), n * H * W <= pixels -> the taps of out (an LpipsFeatures of n)."""
        lib = self._lib
        n, _, H, W = x.shape
        stream = lib.stream_ptr()
        xf, xq = (None, x.data_ptr()) if mode == 2 else (x.data_ptr(), None)
        lib.check(lib.lib.rick_lpips_input_f32(xf, xq, self.x0.data_ptr(), u8out.data_ptr() if u8out is not None else None,
                                               n, H, W, mode, stream), 'rick_lpips_input_f32')

        def invnorm(s, tap, n, h, w):
            lib.check(lib.lib.rick_lpips_invnorm_f32(tap, out.inorm[s].data_ptr(), n * h * w, CHANNELS[s], stream),
                      'rick_lpips_invnorm_f32')
        self.trunk.run(self.x0.data_ptr(), n, H, W, self.bufs, lambda s: out.taps[s].data_ptr(), invnorm)


class LPIPS:
    """lpips 0.1 (VGG16) on HIP kernels; see the module docstring."""

    def __init__(self, convs, lins, device='cuda', batch=25, size=SIZE):
        if batch < 1:
            raise ValueError('LPIPS: batch must be >= 1')
        self.convs, self.lins = convs, lins
        self.batch, self.size = int(batch), int(size)
        self.device = torch.device(device)
        self._plan, self.workspace_features, self._second = None, None, None
        if self.device.type == 'cuda':
            if self.device.index is None:
                self.device = torch.device('cuda', torch.cuda.current_device())
            with torch.cuda.device(self.device):
                self._plan = _Plan(convs, lins, self.batch, self.size, self.device)
                self.workspace_features = LpipsFeatures.empty(self.batch, self.size, self.size, self.device)

    @classmethod
    def load(cls, src=None, device='cuda', batch=25, size=SIZE, vgg=None, lin=None):
        """src: a path or state_dict in the lpips layout; or vgg= (torchvision vgg16) with lin= (lin weights file)."""
        if src is not None:
            if vgg is not None or lin is not None:
                raise ValueError('LPIPS.load: pass either src, or vgg and lin, not both')
            convs, lins = params_from_lpips(_load_dict(src))
        elif vgg is None or lin is None:
            raise ValueError('LPIPS.load: pass src, or both vgg and lin')
        else:
            convs, lins = params_from_vgg(_load_dict(vgg), _load_dict(lin))
        return cls(convs, lins, device=device, batch=batch, size=size)

    def _check_images(self, x, what):
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f'LPIPS: expected {what} [N, 3, H, W], got {tuple(x.shape)}')
        if x.dtype not in (torch.float32, torch.uint8):
            raise RuntimeError(f'LPIPS: {what} must be float32 or uint8, got {x.dtype}')
        if min(x.shape[2:]) < 16:
            raise ValueError(f'LPIPS: images must be at least 16 x 16, got {tuple(x.shape[2:])}')
        if x.device.type != 'cpu' and x.device != self.device:
            raise RuntimeError(f'LPIPS: {what} on {x.device}, network loaded for {self.device}')

    def new_features(self, n, h=None, w=None):
        return LpipsFeatures.empty(n, h or self.size, w or self.size, self.device)

    @torch.no_grad()
    def features(self, x, quantize=False, out=None, u8_out=None):
        """x [N, 3, H, W] fp32 in [-1, 1] (through the PNG round trip if ``quantize``) or uint8 -> LpipsFeatures of N images
        (written into ``out``, which must hold at least N images of the same size, if given).  ``u8_out`` [N, 3, H, W] uint8
        receives the quantised images (``quantize`` only)."""
        self._check_images(x, 'images')
        N, _, H, W = x.shape
        if u8_out is not None and (not quantize or x.dtype != torch.float32 or tuple(u8_out.shape) != tuple(x.shape)
                                   or u8_out.dtype != torch.uint8 or u8_out.device != x.device or not u8_out.is_contiguous()):
            raise RuntimeError('LPIPS.features: u8_out must be a contiguous uint8 tensor shaped like x, with quantize=True')
        dev = x.device
        if out is None:
            out = LpipsFeatures.empty(N, H, W, dev)
        elif out.n < N or out.size != (H, W) or out.device != dev:
            raise RuntimeError(f'LPIPS.features: out holds {out.n} images of {out.size} on {out.device}, need {N} of {(H, W)}')
        if dev.type == 'cpu':
            xs, q = scale_input(x, quantize)
            if u8_out is not None:
                u8_out.copy_(q)
            for s, f in enumerate(_cpu_taps(self.convs, xs)):
                out.taps[s][:N] = f.permute(0, 2, 3, 1)
                out.inorm[s][:N] = _inverse_norm(f, 1).flatten(1)
            return out.narrow(0, N) if out.n != N else out
        if H * W > self._plan.pixels:
            raise ValueError(f'LPIPS: {H} x {W} images exceed the workspace planned for {self.batch} x {self.size}^2')
        mode = 2 if x.dtype == torch.uint8 else int(bool(quantize))
        x = x.contiguous()
        chunk = self._plan.pixels // (H * W)
        with torch.cuda.device(self.device):
            for lo in range(0, N, chunk):
                hi = min(N, lo + chunk)
                self._plan.run(x[lo:hi], mode, out.narrow(lo, hi), None if u8_out is None else u8_out[lo:hi])
        return out.narrow(0, N) if out.n != N else out

    @torch.no_grad()
    def distances(self, fa, fb):
        """[na, nb] fp32: LPIPS between every image of fa and every image of fb (both LpipsFeatures of one size)."""
        if fa.size != fb.size or fa.device != fb.device:
            raise RuntimeError('LPIPS.distances: feature sets of different sizes or devices')
        na, nb = fa.n, fb.n
        if fa.device.type == 'cpu':
            out = torch.zeros(na, nb, dtype=torch.float64)
            for s in range(5):
                a = (fa.taps[s] * fa.inorm[s].view(fa.taps[s].shape[:3])[..., None]).flatten(1, 2)   # [na, HW, C]
                b = (fb.taps[s] * fb.inorm[s].view(fb.taps[s].shape[:3])[..., None]).flatten(1, 2)
                for i in range(na):
                    out[i] += (((a[i:i + 1] - b) ** 2) * self.lins[s]).sum(2).mean(1).double()
            return out.float()
        lib = self._lib()
        hws = [t.shape[1] * t.shape[2] for t in fa.taps]
        nsl = [-(-hw // _positions_per_slice(c)) for hw, c in zip(hws, CHANNELS)]
        out = torch.empty((na, nb), device=fa.device, dtype=torch.float32)
        if na == 0 or nb == 0:
            return out
        part = torch.empty(sum(nsl) * na * nb, device=fa.device, dtype=torch.float64)
        d = lib.LpipsLayers()
        d.nlayers = 5
        with torch.cuda.device(fa.device):
            stream, off = lib.stream_ptr(), 0
            for s in range(5):
                ta, tb = fa.taps[s], fb.taps[s]
                if not (ta.is_contiguous() and tb.is_contiguous() and fa.inorm[s].is_contiguous() and fb.inorm[s].is_contiguous()):
                    raise RuntimeError('LPIPS.distances: feature tensors must be contiguous')
                lib.check(lib.lib.rick_lpips_pair_f32(ta.data_ptr(), fa.inorm[s].data_ptr(), na, tb.data_ptr(),
                                                      fb.inorm[s].data_ptr(), nb, self._plan.lins[s].data_ptr(), hws[s],
                                                      CHANNELS[s], _positions_per_slice(CHANNELS[s]), part[off:].data_ptr(),
                                                      stream), 'rick_lpips_pair_f32')
                d.nslices[s], d.hw[s] = nsl[s], hws[s]
                off += nsl[s] * na * nb
            lib.check(lib.lib.rick_lpips_reduce_f32(part.data_ptr(), out.data_ptr(), na, nb, ctypes.byref(d), stream),
                      'rick_lpips_reduce_f32')
        return out

    @staticmethod
    def _lib():
        from . import _lib
        return _lib

    @torch.no_grad()
    def __call__(self, x, y, quantize=False):
        """Paired LPIPS, like ``lpips_fn(x, y)``: x, y [N, 3, H, W] -> [N] fp32."""
        self._check_images(x, 'x')
        self._check_images(y, 'y')
        if x.shape != y.shape:
            raise RuntimeError(f'LPIPS: x {tuple(x.shape)} and y {tuple(y.shape)} differ')
        N, _, H, W = x.shape
        if x.device.type == 'cpu':
            xs, _ = scale_input(x, quantize)
            ys, _ = scale_input(y, quantize)
            val = 0
            for s, (fx, fy) in enumerate(zip(_cpu_taps(self.convs, xs), _cpu_taps(self.convs, ys))):
                nx = fx / (fx.pow(2).sum(1, keepdim=True).sqrt() + EPS)
                ny = fy / (fy.pow(2).sum(1, keepdim=True).sqrt() + EPS)
                val = val + ((nx - ny) ** 2 * self.lins[s].view(1, -1, 1, 1)).sum(1).mean((1, 2))
            return val
        out = torch.empty(N, device=x.device, dtype=torch.float32)
        if (H, W) == (self.size, self.size):
            fx = self.workspace_features
            if self._second is None:
                self._second = LpipsFeatures.empty(self.batch, self.size, self.size, self.device)
            fy, step = self._second, self.batch
        else:
            step = max(1, min(N, self._plan.pixels // (H * W)))
            fx, fy = LpipsFeatures.empty(step, H, W, self.device), LpipsFeatures.empty(step, H, W, self.device)
        for lo in range(0, N, step):
            hi = min(N, lo + step)
            a = self.features(x[lo:hi], quantize, out=fx)
            b = self.features(y[lo:hi], quantize, out=fy)
            out[lo:hi] = torch.diagonal(self.distances(a, b))
        return out
