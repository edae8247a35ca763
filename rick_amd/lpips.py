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
``paired`` forms only image i against image i (rick_lpips_paired_f32: the same sums in the same order, so the same bits as
the diagonal of ``distances``, for n pairs of work instead of n^2); ``net(x, y)`` and the no-grad ``net.loss`` run on it.

CUDA fp32 inputs run the kernels of rick_amd/csrc/lpips.hip and the Inception convolution rick_inc_conv_f32 (f32-input MFMA,
no split-K: an image's taps are bit-identical whatever batch it is computed in).  The workspace (input, two ping-pong
activation buffers and one tap set of ``batch`` images at ``size`` x ``size``) is allocated once in ``load``.  CPU tensors
run the same network as a plain fp32 torch composition.

``net.loss(x, target)`` is the same paired distance as a loss: differentiable (first order) with respect to the image x,
against a fixed target (an image tensor, or the LpipsFeatures of N images or of one image for all).  On the device the forward
run keeps the 13 activations of the trunk in a workspace of ``batch`` images at ``size`` x ``size`` that is allocated on the
first differentiable call, and the backward pass runs on rick_lpips_tap_bwd_f32 (the distance), rick_inc_conv_bwd_f32 (the
convolutions' data gradients, the transposed filters packed at load), rick_lpips_maxpool2_bwd_f32 (pool adjoint + tap gradient
+ ReLU mask) and rick_lpips_input_bwd_f32.  The weights are constants; the no-grad entries launch what they always did.

``src`` is a path to (or the contents of) either ``lpips.LPIPS(net='vgg').state_dict()`` (``net.slice{1..5}.{idx}.*``,
``lin{k}.model.1.weight``, optionally the ``lins.{k}.*`` duplicates and the ``scaling_layer.*`` buffers), or use
``LPIPS.load(vgg=..., lin=...)`` with a torchvision ``vgg16`` state_dict (``features.{idx}.*``; ``classifier.*`` ignored)
and the lin weights file (``lin{k}.model.1.weight``, the layout of lpips' ``weights/v0.1/vgg.pth``).
"""
import ctypes
import functools

import torch

from .netutil import check_images, cuda_device, get, load_dict
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
_get = functools.partial(get, who='LPIPS')


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
        self.trunk = VggTrunk(convs, device, transposed=True)
        self.x0 = torch.empty(self.pixels * 4, device=device, dtype=torch.float32)
        self.bufs = self.trunk.new_buffers(self.pixels, device)
        self.lins = [w.to(device) for w in lins]

    def run(self, x, mode, out, u8out, keep=None):
        """x [n, 3, H, W] (fp32, or uint8 for mode 2), n * H * W <= pixels -> the taps of out (an LpipsFeatures of n); keep:
        VggTrunk.run's."""
        lib = self._lib
        n, _, H, W = x.shape
        stream = lib.stream_ptr()
        xf, xq = (None, x.data_ptr()) if mode == 2 else (x.data_ptr(), None)
        lib.check(lib.lib.rick_lpips_input_f32(xf, xq, self.x0.data_ptr(), u8out.data_ptr() if u8out is not None else None,
                                               n, H, W, mode, stream), 'rick_lpips_input_f32')

        def invnorm(s, tap, n, h, w):
            lib.check(lib.lib.rick_lpips_invnorm_f32(tap, out.inorm[s].data_ptr(), n * h * w, CHANNELS[s], stream),
                      'rick_lpips_invnorm_f32')
        self.trunk.run(self.x0.data_ptr(), n, H, W, self.bufs, lambda s: out.taps[s].data_ptr(), invnorm, keep=keep)


class _GradWorkspace:
    """What a differentiable call keeps between its forward and its backward run: the 13 activations of the trunk (the five
    stage outputs as an LpipsFeatures with their inverse norms) and three gradient buffers, for `batch` images at size x size
    (any n * H * W up to that).  `version` counts forward runs: a backward run whose activations were overwritten refuses."""

    def __init__(self, plan, device):
        f32 = dict(device=device, dtype=torch.float32)
        self.plan, self.pixels, self.version = plan, plan.pixels, 0
        self.acts, area = [], 1.0
        for s, stage in enumerate(STAGES):
            area = area / 4 if s else area
            self.acts += [torch.empty(int(self.pixels * area * co), **f32) for _, _, co in stage]
        self.inorm = [torch.empty(max(1, self.pixels >> (2 * s)), **f32) for s in range(5)]
        self.gbufs = [torch.empty(self.pixels * 64, **f32) for _ in range(3)]
        self.last = [sum(len(st) for st in STAGES[:s + 1]) - 1 for s in range(5)]

    def features(self, n, h, w):
        """The stage outputs of n images of h x w as views of the workspace."""
        taps = [self.acts[k][:n * a * b * c].view(n, a, b, c) for k, (a, b), c in zip(self.last, _tap_hw(h, w), CHANNELS)]
        return LpipsFeatures(taps, [t[:n * a * b].view(n, a * b) for t, (a, b) in zip(self.inorm, _tap_hw(h, w))])

    def forward(self, x):
        n, _, H, W = x.shape
        f = self.features(n, H, W)
        self.version += 1
        self.plan.run(x, 0, f, None, keep=[t.data_ptr() for t in self.acts])
        return f

    def backward(self, f, target, go, lins, gx):
        """f: this workspace's features of the forward run; go [n] -> gx [n, 3, H, W]."""
        lib = self.plan._lib
        n, (H, W) = f.n, f.size
        stream = lib.stream_ptr()

        def tap_grad(s, ptr, n, h, w, relu):
            lib.check(lib.lib.rick_lpips_tap_bwd_f32(f.taps[s].data_ptr(), f.inorm[s].data_ptr(), target.taps[s].data_ptr(),
                                                     target.inorm[s].data_ptr(), n, target.n, lins[s].data_ptr(),
                                                     go.data_ptr(), h * w, CHANNELS[s], int(relu), ptr, stream),
                      'rick_lpips_tap_bwd_f32')
        g0 = self.plan.trunk.run_backward(n, H, W, [t.data_ptr() for t in self.acts], self.gbufs, tap_grad)
        lib.check(lib.lib.rick_lpips_input_bwd_f32(g0, gx.data_ptr(), n, H, W, stream), 'rick_lpips_input_bwd_f32')


class _LpipsLoss(torch.autograd.Function):
    """[N] paired LPIPS of x against fixed target features; the gradient with respect to x on the HIP backward kernels."""

    @staticmethod
    def forward(ctx, x, net, target):
        ws = net._grad_workspace()
        with torch.cuda.device(net.device):
            f = ws.forward(x)
            d = net.paired(f, target) if target.n == f.n and f.n > 1 else net.distances(f, target)[:, 0].contiguous()
        ctx.net, ctx.target, ctx.f, ctx.version = net, target, f, ws.version
        return d

    @staticmethod
    def backward(ctx, go):
        if torch.is_grad_enabled():
            raise RuntimeError('LPIPS.loss: the backward pass is first order only (create_graph=True is not supported)')
        ws = ctx.net._grad_workspace()
        if ws.version != ctx.version:
            raise RuntimeError('LPIPS.loss: the stored activations were overwritten by a later differentiable call; '
                               'run backward before the next LPIPS.loss on this network')
        if go.device != ctx.net.device or go.dtype != torch.float32:
            raise RuntimeError(f'LPIPS.loss: upstream gradient on {go.device} / {go.dtype}')
        n, (H, W) = ctx.f.n, ctx.f.size
        go = go.contiguous()
        gx = torch.empty((n, 3, H, W), device=go.device, dtype=torch.float32)
        with torch.cuda.device(ctx.net.device):
            ws.backward(ctx.f, ctx.target, go, ctx.net._plan.lins, gx)
        return gx, None, None


class LPIPS:
    """lpips 0.1 (VGG16) on HIP kernels; see the module docstring."""

    def __init__(self, convs, lins, device='cuda', batch=25, size=SIZE):
        if batch < 1:
            raise ValueError('LPIPS: batch must be >= 1')
        self.convs, self.lins = convs, lins
        self.batch, self.size = int(batch), int(size)
        self.device = cuda_device(device)
        self._plan, self.workspace_features, self._second, self._grad_ws = None, None, None, None
        if self.device.type == 'cuda':
            with torch.cuda.device(self.device):
                self._plan = _Plan(convs, lins, self.batch, self.size, self.device)
                self.workspace_features = LpipsFeatures.empty(self.batch, self.size, self.size, self.device)

    @classmethod
    def load(cls, src=None, device='cuda', batch=25, size=SIZE, vgg=None, lin=None):
        """src: a path or state_dict in the lpips layout; or vgg= (torchvision vgg16) with lin= (lin weights file)."""
        if src is not None:
            if vgg is not None or lin is not None:
                raise ValueError('LPIPS.load: pass either src, or vgg and lin, not both')
            convs, lins = params_from_lpips(load_dict(src))
        elif vgg is None or lin is None:
            raise ValueError('LPIPS.load: pass src, or both vgg and lin')
        else:
            convs, lins = params_from_vgg(load_dict(vgg), load_dict(lin))
        return cls(convs, lins, device=device, batch=batch, size=size)

    def _check_images(self, x, what):
        check_images(x, 'LPIPS', self.device, what, dtypes=(torch.float32, torch.uint8), min_size=16)

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

    @torch.no_grad()
    def paired(self, fa, fb=None):
        """[n] fp32: LPIPS between image i of fa and image i of fb (LpipsFeatures of n images each).  With ``fb=None`` the
        pairs are the rows (2i, 2i + 1) of fa, which must hold an even number of images: one feature set serves as both
        operands.  On the device this is rick_lpips_paired_f32 (n pairs of work and partials, not n^2) and every value is
        bit-identical to the diagonal of ``distances``."""
        if fb is None:
            if fa.n % 2:
                raise RuntimeError(f'LPIPS.paired: {fa.n} images cannot be paired as rows (2i, 2i + 1)')
            n, stride = fa.n // 2, 2
        else:
            if fa.size != fb.size or fa.device != fb.device or fa.n != fb.n:
                raise RuntimeError(f'LPIPS.paired: {fa.n} images of {fa.size} on {fa.device} against {fb.n} of {fb.size} on '
                                   f'{fb.device}')
            n, stride = fa.n, 1
        if fa.device.type == 'cpu':
            if fb is None:
                fa, fb = (LpipsFeatures([t[k::2] for t in fa.taps], [t[k::2] for t in fa.inorm]) for k in (0, 1))
            out = torch.zeros(n, dtype=torch.float64)
            for s in range(5):
                a = (fa.taps[s] * fa.inorm[s].view(fa.taps[s].shape[:3])[..., None]).flatten(1, 2)   # [n, HW, C]
                b = (fb.taps[s] * fb.inorm[s].view(fb.taps[s].shape[:3])[..., None]).flatten(1, 2)
                out += (((a - b) ** 2) * self.lins[s]).sum(2).mean(1).double()
            return out.float()
        lib = self._lib()
        hws = [t.shape[1] * t.shape[2] for t in fa.taps]
        nsl = [-(-hw // _positions_per_slice(c)) for hw, c in zip(hws, CHANNELS)]
        out = torch.empty(n, device=fa.device, dtype=torch.float32)
        if n == 0:
            return out
        part = torch.empty(sum(nsl) * n, device=fa.device, dtype=torch.float64)
        d = lib.LpipsLayers()
        d.nlayers = 5
        with torch.cuda.device(fa.device):
            stream, off = lib.stream_ptr(), 0
            for s in range(5):
                sets = (fa,) if fb is None else (fa, fb)
                if not all(f.taps[s].is_contiguous() and f.inorm[s].is_contiguous() for f in sets):
                    raise RuntimeError('LPIPS.paired: feature tensors must be contiguous')
                ta, ia = fa.taps[s].data_ptr(), fa.inorm[s].data_ptr()
                if fb is None:                       # image 2i + 1 lies one image behind image 2i
                    tb, ib = ta + 4 * hws[s] * CHANNELS[s], ia + 4 * hws[s]
                else:
                    tb, ib = fb.taps[s].data_ptr(), fb.inorm[s].data_ptr()
                lib.check(lib.lib.rick_lpips_paired_f32(ta, ia, stride, tb, ib, stride, n, self._plan.lins[s].data_ptr(), hws[s],
                                                        CHANNELS[s], _positions_per_slice(CHANNELS[s]), part[off:].data_ptr(),
                                                        stream), 'rick_lpips_paired_f32')
                d.nslices[s], d.hw[s] = nsl[s], hws[s]
                off += nsl[s] * n
            lib.check(lib.lib.rick_lpips_reduce_f32(part.data_ptr(), out.data_ptr(), n, 1, ctypes.byref(d), stream),
                      'rick_lpips_reduce_f32')
        return out

    @staticmethod
    def _lib():
        from . import _lib
        return _lib

    def _grad_workspace(self):
        if self._grad_ws is None:
            with torch.cuda.device(self.device):
                self._grad_ws = _GradWorkspace(self._plan, self.device)
        return self._grad_ws

    def loss(self, x, target, quantize=False):
        """Paired LPIPS as a loss: x [N, 3, H, W] fp32 (may require grad) against ``target``, an LpipsFeatures of N images
        or of 1 image (compared with every x), or an image tensor of N or 1 images (its features are taken without a
        gradient) -> [N] fp32, bit-identical to ``net(x, y)``.  Differentiable with respect to x only, first order only:
        ``create_graph=True`` raises in the backward pass.  ``quantize`` (the PNG round trip) has no gradient: with an x that
        requires one it raises.  On the device a differentiable call takes N * H * W <= batch * size^2, and its backward
        pass must run before the next differentiable call on this network (one set of stored activations)."""
        self._check_images(x, 'x')
        if x.dtype != torch.float32:
            raise RuntimeError(f'LPIPS.loss: x must be float32, got {x.dtype}')
        needs_grad = torch.is_grad_enabled() and x.requires_grad
        if quantize and needs_grad:
            raise RuntimeError('LPIPS.loss: quantize=True rounds x to uint8 and has no gradient; pass quantize=False')
        if torch.is_tensor(target):
            target = self.features(target.detach(), quantize)
        N, _, H, W = x.shape
        if target.n not in (N, 1) or target.size != (H, W) or target.device != x.device:
            raise RuntimeError(f'LPIPS.loss: target holds {target.n} images of {target.size} on {target.device}, x is '
                               f'{N} of {(H, W)} on {x.device}')
        if x.device.type == 'cpu':
            xs, _ = scale_input(x, quantize)
            val = 0
            for s, fx in enumerate(_cpu_taps(self.convs, xs)):
                ss = fx.pow(2).sum(1, keepdim=True)            # an all-zero position: 0 and gradient 0, as on the device
                nx = torch.where(ss > 0, fx / (torch.where(ss > 0, ss, torch.ones_like(ss)).sqrt() + EPS), torch.zeros_like(fx))
                ny = (target.taps[s] * target.inorm[s].view(target.taps[s].shape[:3])[..., None]).permute(0, 3, 1, 2)
                val = val + ((nx - ny) ** 2 * self.lins[s].view(1, -1, 1, 1)).sum(1).mean((1, 2))
            return val
        if not needs_grad:
            f = self.features(x, quantize)
            return self.paired(f, target) if target.n == N and N > 1 else self.distances(f, target)[:, 0].contiguous()
        if N * H * W > self._plan.pixels:
            raise ValueError(f'LPIPS.loss: {N} images of {H} x {W} exceed the workspace planned for {self.batch} x '
                             f'{self.size}^2')
        if not all(t.is_contiguous() for t in target.taps + target.inorm):
            raise RuntimeError('LPIPS.loss: target feature tensors must be contiguous')
        return _LpipsLoss.apply(x.contiguous(), self, target)

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
            out[lo:hi] = self.paired(a, b)
        return out
