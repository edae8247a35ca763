"""InceptionV3 pool3 features on HIP kernels: the network behind the reference's FID (gan_training/metrics/inception.py,
fid_score.py), as a ``feature_fn`` for ``rick_amd.evaluate``.

    net = InceptionV3Features.load(src, device='cuda', dims=2048, batch=100)
    feats = net(images)        # images [N, 3, H, W] fp32 in [-1, 1], any H, W  ->  [N, dims] fp32

``src`` is a path to (or the contents of) torchvision's ``Inception3`` ImageNet state_dict, or of the reference wrapper
``InceptionV3`` (``blocks.<i>.<j>.…``).  The computation is the wrapper's (inception.py:83-106): bilinear resize to 299 x 299
(``F.interpolate(align_corners=False)``, what ``F.upsample`` did), the ImageNet affine, torchvision's blocks up to the one
``dims`` selects, and a global average pool (fid_score.py:83-84 for ``dims`` 64 / 192 / 768).

Every BasicConv2d is conv -> BatchNorm(eps 1e-3) -> ReLU; the BN is folded into the convolution (in fp64, stored fp32) when
the weights are loaded.  CUDA fp32 inputs run the HIP kernels of rick_amd/csrc/inception.hip (NHWC activations, one
f32-input MFMA implicit GEMM per convolution, the 1x1 heads that share an input fused into one GEMM, concats written in
place; operands, descriptors and launches by rick_amd/gemm_conv.py, the classifier's by rick_amd/fc.py); CPU inputs run the
same folded network as a plain fp32 torch composition.  The CUDA path is capture-safe at a
fixed N: the workspace is allocated once in ``load``, every launch goes to the caller's stream, branches run in order.

``InceptionV3Logits`` is the same trunk with torchvision's classifier head, the network behind the reference's Inception Score
(gan_training/metrics/inception_score.py): ``inception_v3(transform_input=False)`` on the images as they are, or after a
bilinear resize to 299 x 299, then pool3 -> ``fc`` 2048 -> 1000.

    net = InceptionV3Logits.load(src, device='cuda', batch=100, size=None)      # size=(H, W): no resize, that size only
    logits = net(images)       # [N, 1000] fp32
    p = net.probs(images)      # fp32 softmax of the rows

The launch plan takes its geometry from the input size (75 x 75 at least, torchvision's floor; H and W may differ) and sizes
its buffers from a dry walk over the layer table.
"""
import re

import torch
import torch.nn.functional as F

from . import fc as fc_ops
from . import gemm_conv
from .gemm_conv import out_hw as _out_hw
from .netutil import check_images, cuda_device, get, load_dict

EPS = 1e-3
SIZE = 299
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
BLOCK_BY_DIMS = {64: 0, 192: 1, 768: 2, 2048: 3}

# ---- the layer table (torchvision Inception3 up to Mixed_7c) ------------------------------------------------------------
# unit: (name, Ci, Co, (kh, kw), (sh, sw), (ph, pw))
STEM0 = [('Conv2d_1a_3x3', 3, 32, (3, 3), (2, 2), (0, 0)), ('Conv2d_2a_3x3', 32, 32, (3, 3), (1, 1), (0, 0)),
         ('Conv2d_2b_3x3', 32, 64, (3, 3), (1, 1), (1, 1))]
STEM1 = [('Conv2d_3b_1x1', 64, 80, (1, 1), (1, 1), (0, 0)), ('Conv2d_4a_3x3', 80, 192, (3, 3), (1, 1), (0, 0))]
# (kind, name, in channels, kind parameter): A -> pool features, C -> c7, E -> -
MIXED = [('A', 'Mixed_5b', 192, 32), ('A', 'Mixed_5c', 256, 64), ('A', 'Mixed_5d', 288, 64), ('B', 'Mixed_6a', 288, None),
         ('C', 'Mixed_6b', 768, 128), ('C', 'Mixed_6c', 768, 160), ('C', 'Mixed_6d', 768, 160), ('C', 'Mixed_6e', 768, 192),
         ('D', 'Mixed_7a', 768, None), ('E', 'Mixed_7b', 1280, None), ('E', 'Mixed_7c', 2048, None)]
MIXED_BLOCK = {'Mixed_5b': 2, 'Mixed_5c': 2, 'Mixed_5d': 2, 'Mixed_6a': 2, 'Mixed_6b': 2, 'Mixed_6c': 2, 'Mixed_6d': 2,
               'Mixed_6e': 2, 'Mixed_7a': 3, 'Mixed_7b': 3, 'Mixed_7c': 3}
# the reference wrapper's blocks.<i>.<j> -> torchvision module (inception.py:36-76)
WRAPPER = {(0, 0): 'Conv2d_1a_3x3', (0, 1): 'Conv2d_2a_3x3', (0, 2): 'Conv2d_2b_3x3', (1, 0): 'Conv2d_3b_1x1',
           (1, 1): 'Conv2d_4a_3x3', (2, 0): 'Mixed_5b', (2, 1): 'Mixed_5c', (2, 2): 'Mixed_5d', (2, 3): 'Mixed_6a',
           (2, 4): 'Mixed_6b', (2, 5): 'Mixed_6c', (2, 6): 'Mixed_6d', (2, 7): 'Mixed_6e', (3, 0): 'Mixed_7a',
           (3, 1): 'Mixed_7b', (3, 2): 'Mixed_7c'}
TENSORS = ('conv.weight', 'bn.weight', 'bn.bias', 'bn.running_mean', 'bn.running_var')
IGNORED = re.compile(r'^(AuxLogits\.|fc\.)|\.num_batches_tracked$')


def mixed_units(kind, name, cin, par):
    """BasicConv2d units of one Inception block, in torchvision's definition order."""
    u = lambda b, ci, co, k=(1, 1), s=(1, 1), p=(0, 0): (f'{name}.{b}', ci, co, k, s, p)   # noqa: E731
    if kind == 'A':
        return [u('branch1x1', cin, 64), u('branch5x5_1', cin, 48), u('branch5x5_2', 48, 64, (5, 5), p=(2, 2)),
                u('branch3x3dbl_1', cin, 64), u('branch3x3dbl_2', 64, 96, (3, 3), p=(1, 1)),
                u('branch3x3dbl_3', 96, 96, (3, 3), p=(1, 1)), u('branch_pool', cin, par)]
    if kind == 'B':
        return [u('branch3x3', cin, 384, (3, 3), (2, 2)), u('branch3x3dbl_1', cin, 64),
                u('branch3x3dbl_2', 64, 96, (3, 3), p=(1, 1)), u('branch3x3dbl_3', 96, 96, (3, 3), (2, 2))]
    if kind == 'C':
        c7 = par
        return [u('branch1x1', cin, 192), u('branch7x7_1', cin, c7), u('branch7x7_2', c7, c7, (1, 7), p=(0, 3)),
                u('branch7x7_3', c7, 192, (7, 1), p=(3, 0)), u('branch7x7dbl_1', cin, c7),
                u('branch7x7dbl_2', c7, c7, (7, 1), p=(3, 0)), u('branch7x7dbl_3', c7, c7, (1, 7), p=(0, 3)),
                u('branch7x7dbl_4', c7, c7, (7, 1), p=(3, 0)), u('branch7x7dbl_5', c7, 192, (1, 7), p=(0, 3)),
                u('branch_pool', cin, 192)]
    if kind == 'D':
        return [u('branch3x3_1', cin, 192), u('branch3x3_2', 192, 320, (3, 3), (2, 2)), u('branch7x7x3_1', cin, 192),
                u('branch7x7x3_2', 192, 192, (1, 7), p=(0, 3)), u('branch7x7x3_3', 192, 192, (7, 1), p=(3, 0)),
                u('branch7x7x3_4', 192, 192, (3, 3), (2, 2))]
    return [u('branch1x1', cin, 320), u('branch3x3_1', cin, 384), u('branch3x3_2a', 384, 384, (1, 3), p=(0, 1)),
            u('branch3x3_2b', 384, 384, (3, 1), p=(1, 0)), u('branch3x3dbl_1', cin, 448),
            u('branch3x3dbl_2', 448, 384, (3, 3), p=(1, 1)), u('branch3x3dbl_3a', 384, 384, (1, 3), p=(0, 1)),
            u('branch3x3dbl_3b', 384, 384, (3, 1), p=(1, 0)), u('branch_pool', cin, 192)]


def units(last_block=3):
    """[(name, Ci, Co, k, s, p)] of every BasicConv2d up to block `last_block`, in network order (94 for block 3)."""
    out = list(STEM0)
    if last_block >= 1:
        out += STEM1
    for kind, name, cin, par in MIXED:
        if MIXED_BLOCK[name] <= last_block:
            out += mixed_units(kind, name, cin, par)
    return out


def expected_keys(last_block=3):
    """torchvision state_dict keys the extractor reads (5 per unit)."""
    return {f'{u[0]}.{t}' for u in units(last_block) for t in TENSORS}


def canonical_state_dict(sd):
    """torchvision key layout from either layout; AuxLogits.*, fc.* and *.num_batches_tracked dropped."""
    out = {}
    for k, v in sd.items():
        m = re.match(r'^blocks\.(\d+)\.(\d+)\.(.*)$', k)
        if m:
            mod = WRAPPER.get((int(m.group(1)), int(m.group(2))))
            if mod is None:                     # the wrapper's pooling layers have no parameters
                raise KeyError(f'InceptionV3Features: unexpected key {k!r}')
            k = f'{mod}.{m.group(3)}'
        if IGNORED.search(k):
            continue
        out[k] = v
    return out


def fold(sd, last_block=3):
    """{unit: (w[Co, Ci, kh, kw], b[Co])} fp32 on the CPU: BatchNorm folded in fp64.  A missing or mis-shaped key is an
    error that names it."""
    sd = canonical_state_dict(sd)
    need = expected_keys(last_block)
    extra = sorted(k for k in sd if k not in expected_keys(3))
    if extra:
        raise KeyError(f'InceptionV3Features: unexpected key {extra[0]!r}')
    folded = {}
    for name, ci, co, (kh, kw), _, _ in units(last_block):
        t = {suffix: get(sd, f'{name}.{suffix}', (co, ci, kh, kw) if suffix == 'conv.weight' else (co,), 'InceptionV3Features',
                         dtype=torch.float64) for suffix in TENSORS}
        scale = t['bn.weight'] / torch.sqrt(t['bn.running_var'] + EPS)
        w = t['conv.weight'] * scale[:, None, None, None]
        b = t['bn.bias'] - t['bn.running_mean'] * scale
        folded[name] = (w.float().contiguous(), b.float().contiguous())
    assert set(f'{n}.{s}' for n in folded for s in TENSORS) == need
    return folded


# ---- CPU: the folded network as an fp32 torch composition ---------------------------------------------------------------
def _cpu_forward(P, x, last_block, affine=True):
    """affine=True: the FID wrapper's resize to 299 and ImageNet affine first; False: the blocks on x as it is."""
    def conv(name, v, s=(1, 1), p=(0, 0)):
        w, b = P[name]
        return F.relu(F.conv2d(v, w, b, s, p))

    def unit(u, v):
        return conv(u[0], v, u[4], u[5])

    def pool(v):
        return F.avg_pool2d(v, 3, 1, 1, count_include_pad=True)

    if affine:
        x = F.interpolate(x, (SIZE, SIZE), mode='bilinear', align_corners=False)
        x = torch.cat([x[:, c:c + 1] * (STD[c] / 0.5) + (MEAN[c] - 0.5) / 0.5 for c in range(3)], 1)
    for u in STEM0:
        x = unit(u, x)
    x = F.max_pool2d(x, 3, 2)
    if last_block == 0:
        return x.mean((2, 3))
    for u in STEM1:
        x = unit(u, x)
    x = F.max_pool2d(x, 3, 2)
    if last_block == 1:
        return x.mean((2, 3))
    for kind, name, cin, par in MIXED:
        if MIXED_BLOCK[name] > last_block:
            break
        U = {u[0].split('.', 1)[1]: u for u in mixed_units(kind, name, cin, par)}
        f = lambda b, v: unit(U[b], v)     # noqa: E731
        if kind == 'A':
            x = torch.cat([f('branch1x1', x), f('branch5x5_2', f('branch5x5_1', x)),
                           f('branch3x3dbl_3', f('branch3x3dbl_2', f('branch3x3dbl_1', x))), f('branch_pool', pool(x))], 1)
        elif kind == 'B':
            x = torch.cat([f('branch3x3', x), f('branch3x3dbl_3', f('branch3x3dbl_2', f('branch3x3dbl_1', x))),
                           F.max_pool2d(x, 3, 2)], 1)
        elif kind == 'C':
            b7 = f('branch7x7_3', f('branch7x7_2', f('branch7x7_1', x)))
            d = x
            for i in range(1, 6):
                d = f(f'branch7x7dbl_{i}', d)
            x = torch.cat([f('branch1x1', x), b7, d, f('branch_pool', pool(x))], 1)
        elif kind == 'D':
            b7 = x
            for i in range(1, 5):
                b7 = f(f'branch7x7x3_{i}', b7)
            x = torch.cat([f('branch3x3_2', f('branch3x3_1', x)), b7, F.max_pool2d(x, 3, 2)], 1)
        else:
            t3 = f('branch3x3_1', x)
            td = f('branch3x3dbl_2', f('branch3x3dbl_1', x))
            x = torch.cat([f('branch1x1', x), f('branch3x3_2a', t3), f('branch3x3_2b', t3), f('branch3x3dbl_3a', td),
                           f('branch3x3dbl_3b', td), f('branch_pool', pool(x))], 1)
    return x.mean((2, 3))


# ---- CUDA: a launch plan over a workspace allocated once ----------------------------------------------------------------
MIN_SIZE = 75                   # torchvision's floor: below it a stride-2 stage has no output left


class _Plan:
    """Buffers and launches of one network at batch `batch` on inputs resized to (or given at) in_hw = (H, W).  Each step is
    f(n, stream).  The layer table is walked twice: a dry walk that only records how many floats each buffer must hold (the
    two ping-pong buffers and every scratch key), then, with the buffers allocated at those sizes, the walk that packs the
    weights and records the launches."""

    def __init__(self, P, last_block, batch, device, in_hw=(SIZE, SIZE), input_kernel='rick_inc_input_f32'):
        from . import _lib
        self._lib = _lib
        self.dev, self.batch, self.steps, self.keep = device, batch, [], []
        self.in_hw, self.input_kernel = (int(in_hw[0]), int(in_hw[1])), input_kernel
        if min(self.in_hw) < MIN_SIZE:
            raise ValueError(f'InceptionV3: the network needs an input of at least {MIN_SIZE} x {MIN_SIZE}, got {self.in_hw}')
        f32 = dict(device=device, dtype=torch.float32)
        self._need, self._bufs = {}, None
        self._walk(P, last_block)                      # dry: sizes only
        self._bufs = {k: torch.empty(n, **f32) for k, n in self._need.items()}
        self.keep += list(self._bufs.values())
        self.x0 = self._bufs['x0']
        self.final, self.final_hw, self.final_c = self._walk(P, last_block)

    def _buf(self, key, numel):
        """The buffer `key`, holding at least `numel` floats (dry walk: its key, and the size is recorded)."""
        if self._bufs is None:
            self._need[key] = max(self._need.get(key, 0), numel)
            return key
        assert self._bufs[key].numel() >= numel
        return self._bufs[key]

    def _walk(self, P, last_block):
        B = self.batch
        scratch = self._buf
        # stem: x0 -> 1a -> 2a -> 2b -> maxpool -> (3b -> 4a -> maxpool)
        (h, w), c = self.in_hw, 4
        cur = self._buf('x0', B * h * w * 4)
        flip = 0
        for stem in ([STEM0] + ([STEM1] if last_block >= 1 else [])):
            for u in stem:
                oh, ow = _out_hw(h, w, u[3], u[4], u[5])
                dst = self._buf(('pp', flip), B * oh * ow * u[2])
                self._conv([u], P, cur, h, w, c, [(dst, u[2], 0)])
                cur, h, w, c, flip = dst, oh, ow, u[2], 1 - flip
            oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            dst = self._buf(('pp', flip), B * oh * ow * c)
            self._maxpool(cur, h, w, c, dst, c, 0)
            cur, h, w, flip = dst, oh, ow, 1 - flip
        for kind, name, cin, par in MIXED:
            if MIXED_BLOCK[name] > last_block:
                break
            U = {u[0].split('.', 1)[1]: u for u in mixed_units(kind, name, cin, par)}
            hw = h * w
            oh, ow = _out_hw(h, w, (3, 3), (2, 2), (0, 0)) if kind in ('B', 'D') else (h, w)
            co = {'A': 224 + (par or 0), 'B': 480 + c, 'C': 768, 'D': 512 + c, 'E': 2048}[kind]
            out = self._buf(('pp', flip), B * oh * ow * co)
            if kind == 'A':
                t5, d1, d2 = scratch('a5', B * hw * 48), scratch('ad1', B * hw * 64), scratch('ad2', B * hw * 96)
                self._conv([U['branch1x1'], U['branch5x5_1'], U['branch3x3dbl_1']], P, cur, h, w, c,
                           [(out, co, 0), (t5, 48, 0), (d1, 64, 0)])
                self._conv([U['branch5x5_2']], P, t5, h, w, 48, [(out, co, 64)])
                self._conv([U['branch3x3dbl_2']], P, d1, h, w, 64, [(d2, 96, 0)])
                self._conv([U['branch3x3dbl_3']], P, d2, h, w, 96, [(out, co, 128)])
                pl = scratch('pool', B * hw * c)
                self._avgpool(cur, h, w, c, pl)
                self._conv([U['branch_pool']], P, pl, h, w, c, [(out, co, 224)])
            elif kind == 'B':
                d1, d2 = scratch('ad1', B * hw * 64), scratch('ad2', B * hw * 96)
                self._conv([U['branch3x3']], P, cur, h, w, c, [(out, co, 0)])
                self._conv([U['branch3x3dbl_1']], P, cur, h, w, c, [(d1, 64, 0)])
                self._conv([U['branch3x3dbl_2']], P, d1, h, w, 64, [(d2, 96, 0)])
                self._conv([U['branch3x3dbl_3']], P, d2, h, w, 96, [(out, co, 384)])
                self._maxpool(cur, h, w, c, out, co, 480)
            elif kind == 'C':
                c7 = par
                ta, tb = scratch('c7a', B * hw * 192), scratch('c7b', B * hw * 192)
                da, db = scratch('cda', B * hw * 192), scratch('cdb', B * hw * 192)
                self._conv([U['branch1x1'], U['branch7x7_1'], U['branch7x7dbl_1']], P, cur, h, w, c,
                           [(out, co, 0), (ta, c7, 0), (da, c7, 0)])
                self._conv([U['branch7x7_2']], P, ta, h, w, c7, [(tb, c7, 0)])
                self._conv([U['branch7x7_3']], P, tb, h, w, c7, [(out, co, 192)])
                self._conv([U['branch7x7dbl_2']], P, da, h, w, c7, [(db, c7, 0)])
                self._conv([U['branch7x7dbl_3']], P, db, h, w, c7, [(da, c7, 0)])
                self._conv([U['branch7x7dbl_4']], P, da, h, w, c7, [(db, c7, 0)])
                self._conv([U['branch7x7dbl_5']], P, db, h, w, c7, [(out, co, 384)])
                pl = scratch('pool', B * hw * c)
                self._avgpool(cur, h, w, c, pl)
                self._conv([U['branch_pool']], P, pl, h, w, c, [(out, co, 576)])
            elif kind == 'D':
                t3, ta, tb = scratch('c7a', B * hw * 192), scratch('cda', B * hw * 192), scratch('cdb', B * hw * 192)
                self._conv([U['branch3x3_1'], U['branch7x7x3_1']], P, cur, h, w, c, [(t3, 192, 0), (ta, 192, 0)])
                self._conv([U['branch3x3_2']], P, t3, h, w, 192, [(out, co, 0)])
                self._conv([U['branch7x7x3_2']], P, ta, h, w, 192, [(tb, 192, 0)])
                self._conv([U['branch7x7x3_3']], P, tb, h, w, 192, [(ta, 192, 0)])
                self._conv([U['branch7x7x3_4']], P, ta, h, w, 192, [(out, co, 320)])
                self._maxpool(cur, h, w, c, out, co, 512)
            else:
                t3, d1, d2 = scratch('e3', B * hw * 384), scratch('ed1', B * hw * 448), scratch('ed2', B * hw * 384)
                self._conv([U['branch1x1'], U['branch3x3_1'], U['branch3x3dbl_1']], P, cur, h, w, c,
                           [(out, co, 0), (t3, 384, 0), (d1, 448, 0)])
                self._conv([U['branch3x3_2a']], P, t3, h, w, 384, [(out, co, 320)])
                self._conv([U['branch3x3_2b']], P, t3, h, w, 384, [(out, co, 704)])
                self._conv([U['branch3x3dbl_2']], P, d1, h, w, 448, [(d2, 384, 0)])
                self._conv([U['branch3x3dbl_3a']], P, d2, h, w, 384, [(out, co, 1088)])
                self._conv([U['branch3x3dbl_3b']], P, d2, h, w, 384, [(out, co, 1472)])
                pl = scratch('pool', B * hw * c)
                self._avgpool(cur, h, w, c, pl)
                self._conv([U['branch_pool']], P, pl, h, w, c, [(out, co, 1856)])
            cur, h, w, c, flip = out, oh, ow, co, 1 - flip
        return cur, h * w, c

    def _conv(self, us, P, src, h, w, ci, dsts):
        """One GEMM for the units `us` (same input, same geometry); dsts[i] = (tensor, ldc, c0) of unit i.  The descriptor is
        built here, once; a run only sets its N."""
        k, s, p = us[0][3], us[0][4], us[0][5]
        assert all(u[3] == k and u[4] == s and u[5] == p for u in us)
        if self._bufs is None:
            return
        wpk, bp, cop, bn = gemm_conv.pack(torch.cat([P[u[0]][0] for u in us]), torch.cat([P[u[0]][1] for u in us]), ci_pad=ci)
        wpk, bp = wpk.to(self.dev), bp.to(self.dev)
        self.keep += [wpk, bp]
        a = gemm_conv.descriptor(self.batch, h, w, ci, k, s, p, cop, bn,
                                 [(t.data_ptr(), ldc, c0, u[2]) for (t, ldc, c0), u in zip(dsts, us)])
        in_ptr, w_ptr, b_ptr = src.data_ptr(), wpk.data_ptr(), bp.data_ptr()

        def run(n, stream):
            a.N = n
            gemm_conv.forward(in_ptr, w_ptr, b_ptr, a, stream)
        self.steps.append(run)

    def _maxpool(self, src, h, w, c, dst, ldc, c0):
        if self._bufs is None:
            return
        lib, sp, dp = self._lib, src.data_ptr(), dst.data_ptr()
        self.steps.append(lambda n, stream: lib.check(lib.lib.rick_inc_maxpool_f32(sp, dp, n, h, w, c, ldc, c0, stream),
                                                      'rick_inc_maxpool_f32'))

    def _avgpool(self, src, h, w, c, dst):
        if self._bufs is None:
            return
        lib, sp, dp = self._lib, src.data_ptr(), dst.data_ptr()
        self.steps.append(lambda n, stream: lib.check(lib.lib.rick_inc_avgpool_f32(sp, dp, n, h, w, c, stream),
                                                      'rick_inc_avgpool_f32'))

    def run(self, x, out):
        """x [n, 3, H, W] contiguous fp32 (n <= batch) -> out [n, dims] (a contiguous slice)."""
        lib = self._lib
        n, _, H, W = x.shape
        stream = lib.stream_ptr()
        lib.check(getattr(lib.lib, self.input_kernel)(x.data_ptr(), self.x0.data_ptr(), n, H, W, self.in_hw[0], self.in_hw[1],
                                                      stream), self.input_kernel)
        for step in self.steps:
            step(n, stream)
        lib.check(lib.lib.rick_inc_mean_f32(self.final.data_ptr(), out.data_ptr(), n, self.final_hw, self.final_c, stream),
                  'rick_inc_mean_f32')


class InceptionV3Features:
    """Callable feature extractor: images [N, 3, H, W] in [-1, 1] -> [N, dims] (see the module docstring)."""

    def __init__(self, folded, device='cuda', dims=2048, batch=100):
        if dims not in BLOCK_BY_DIMS:
            raise ValueError(f'InceptionV3Features: dims must be one of {sorted(BLOCK_BY_DIMS)}, got {dims}')
        if batch < 1:
            raise ValueError('InceptionV3Features: batch must be >= 1')
        self.dims, self.batch, self.block = dims, int(batch), BLOCK_BY_DIMS[dims]
        self.folded = folded
        self.device = cuda_device(device)
        self._plan = None
        if self.device.type == 'cuda':
            with torch.cuda.device(self.device):
                self._plan = _Plan(folded, self.block, self.batch, self.device)

    @classmethod
    def load(cls, src, device='cuda', dims=2048, batch=100):
        """src: a path (torch.load, weights_only) or a state_dict, torchvision or reference-wrapper layout."""
        if dims not in BLOCK_BY_DIMS:
            raise ValueError(f'InceptionV3Features: dims must be one of {sorted(BLOCK_BY_DIMS)}, got {dims}')
        return cls(fold(load_dict(src), BLOCK_BY_DIMS[dims]), device=device, dims=dims, batch=batch)

    def __call__(self, images):
        check_images(images, 'InceptionV3Features', self.device, noun='extractor')
        if images.device.type == 'cpu':
            with torch.no_grad():
                return _cpu_forward(self.folded, images, self.block)
        x = images.detach().contiguous()
        N = x.shape[0]
        out = torch.empty((N, self.dims), device=x.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            for lo in range(0, N, self.batch):
                hi = min(N, lo + self.batch)
                self._plan.run(x[lo:hi], out[lo:hi])
        return out


# ---- the classifier head: the Inception Score's network ------------------------------------------------------------------
CLASSES, POOL3 = 1000, 2048


def fc_from_state_dict(sd):
    """(fc.weight [1000, 2048], fc.bias [1000]) fp32 on the CPU; a missing or mis-shaped key is an error that names it."""
    return (get(sd, 'fc.weight', (CLASSES, POOL3), 'InceptionV3Logits'), get(sd, 'fc.bias', (CLASSES,), 'InceptionV3Logits'))


def softmax_rows(logits):
    """logits [M, C] fp32 on the device -> (p [M, C] fp32, s [M] fp64, h [M] fp64) by rick_is_rows_f32: the fp32 softmax, its
    fp64 row sums and the rows' sum q log q with q = p / s."""
    from . import _lib as lib
    lib.require_cuda_f32(logits)
    if logits.dim() != 2 or logits.shape[1] < 1:
        raise RuntimeError(f'softmax_rows: expected logits [M, C], got {tuple(logits.shape)}')
    x = logits.detach().contiguous()
    M, C = x.shape
    p = torch.empty_like(x)
    s = torch.empty(M, device=x.device, dtype=torch.float64)
    h = torch.empty(M, device=x.device, dtype=torch.float64)
    with torch.cuda.device(x.device):
        lib.check(lib.lib.rick_is_rows_f32(x.data_ptr(), p.data_ptr(), s.data_ptr(), h.data_ptr(), M, C, lib.stream_ptr()),
                  'rick_is_rows_f32')
    return p, s, h


def accumulate_rows(acc, p, s, h, row0, per):
    """Fold the rows (p, s, h) of softmax_rows, rows row0 ... of the sample, into acc [S, 2 C + 1] fp64 (rick_is_accum_f64)."""
    from . import _lib as lib
    M, C = p.shape
    if acc.dtype != torch.float64 or not acc.is_contiguous() or acc.dim() != 2 or acc.shape[1] != 2 * C + 1:
        raise RuntimeError(f'accumulate_rows: acc must be contiguous fp64 [S, {2 * C + 1}], got {acc.dtype} {tuple(acc.shape)}')
    if not (p.is_contiguous() and s.is_contiguous() and h.is_contiguous()) or s.numel() != M or h.numel() != M:
        raise RuntimeError('accumulate_rows: p [M, C], s [M] and h [M] must be contiguous')
    if not (p.device == s.device == h.device == acc.device) or s.dtype != torch.float64 or h.dtype != torch.float64:
        raise RuntimeError('accumulate_rows: p fp32, s and h fp64, all on the device of acc')
    lib.require_cuda_f32(p)
    with torch.cuda.device(p.device):
        lib.check(lib.lib.rick_is_accum_f64(p.data_ptr(), s.data_ptr(), h.data_ptr(), acc.data_ptr(), M, C, acc.shape[0],
                                            int(row0), int(per), lib.stream_ptr()), 'rick_is_accum_f64')


class InceptionV3Logits:
    """torchvision's Inception3 (eval, transform_input=False) up to its logits: images [N, 3, H, W] -> [N, 1000] fp32.

    size=None: the images are resized to 299 x 299 (bilinear, align_corners=False), the reference's resize=True.
    size=(H, W): they are taken as they are and must have that size (resize=False)."""

    def __init__(self, folded, fc, device='cuda', batch=100, size=None):
        if batch < 1:
            raise ValueError('InceptionV3Logits: batch must be >= 1')
        self.folded, self.fc, self.batch = folded, fc, int(batch)
        self.size = None if size is None else (int(size[0]), int(size[1]))
        if self.size is not None and min(self.size) < MIN_SIZE:
            raise ValueError(f'InceptionV3Logits: size must be at least {MIN_SIZE} x {MIN_SIZE}, got {self.size}')
        self.classes = CLASSES
        self.device = cuda_device(device)
        self._plan = None
        if self.device.type == 'cuda':
            from . import _lib
            with torch.cuda.device(self.device):
                self._plan = _Plan(folded, 3, self.batch, self.device, in_hw=self.size or (SIZE, SIZE),
                                   input_kernel='rick_inc_input_raw_f32')
                wpk = fc_ops.pack_fc_weight(fc[0])
                fc_ops.check_packed(wpk, POOL3, CLASSES, 'InceptionV3Logits')
                self._wpk, self._bias = wpk.to(self.device), fc[1].to(self.device)
                self._pool3 = torch.empty(self.batch * POOL3, device=self.device, dtype=torch.float32)
                rows = min(self.batch, fc_ops.FC_MAX_ROWS)
                self._ws = torch.empty(_lib.lib.rick_fc_workspace_floats(rows, POOL3, CLASSES), device=self.device,
                                       dtype=torch.float32)

    @classmethod
    def load(cls, src, device='cuda', batch=100, size=None):
        """src: a path (torch.load, weights_only) or a state_dict, torchvision or reference-wrapper layout, with fc.weight and
        fc.bias."""
        src = load_dict(src)
        return cls(fold(src, 3), fc_from_state_dict(src), device=device, batch=batch, size=size)

    def _run_fc(self, n, out):
        """Rows [0, n) of the pool3 workspace through the classifier -> the same rows of out."""
        fc_ops.run_fc(self._pool3.data_ptr(), self._wpk.data_ptr(), self._bias.data_ptr(), self._ws.data_ptr(), out.data_ptr(), n,
                      POOL3, CLASSES, 0)

    def _run(self, x, out):
        """x [n, 3, H, W] contiguous (n <= batch) -> out [n, 1000]: the trunk, pool3 into the workspace, fc in chunks of 64 rows."""
        self._plan.run(x, self._pool3)
        self._run_fc(x.shape[0], out)

    @torch.no_grad()
    def __call__(self, images):
        check_images(images, 'InceptionV3Logits', self.device)
        if self.size is not None and tuple(images.shape[2:]) != self.size:
            raise RuntimeError(f'InceptionV3Logits: loaded for images of {self.size}, got {tuple(images.shape[2:])}')
        if images.device.type == 'cpu':
            out = torch.empty((images.shape[0], CLASSES), dtype=torch.float32)
            for lo in range(0, images.shape[0], self.batch):
                x = images[lo:lo + self.batch]
                if self.size is None:
                    x = F.interpolate(x, (SIZE, SIZE), mode='bilinear', align_corners=False)
                out[lo:lo + self.batch] = F.linear(_cpu_forward(self.folded, x, 3, affine=False), *self.fc)
            return out
        x = images.detach().contiguous()
        N = x.shape[0]
        out = torch.empty((N, CLASSES), device=x.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            for lo in range(0, N, self.batch):
                hi = min(N, lo + self.batch)
                self._run(x[lo:hi], out[lo:hi])
        return out

    @torch.no_grad()
    def probs(self, images):
        """softmax(logits) [N, 1000] fp32: rick_is_rows_f32 on the device, F.softmax on CPU tensors."""
        logits = self(images)
        if logits.device.type == 'cpu':
            return F.softmax(logits, dim=-1)
        return softmax_rows(logits)[0]
