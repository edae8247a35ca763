"""DINOv2's ViT (Oquab et al., 2023) on HIP kernels: the final LayerNorm's class token (transformers' ``pooler_output``), the
feature space of FD-DINOv2 (Stein et al., 2023): the Frechet distance that tracks human judgement where Inception-FID does not.
Forward only, frozen weights.

    net = Dinov2Features.load(src, device='cuda', batch=25, size=224)     # src: a state_dict or a path, either layout below
    f = net(x)                                  # x [N, 3, H, W] fp32 in [-1, 1] -> [N, Wd] fp32 on x's device
    ev = Evaluator(g_ema, net, net(real_images))                          # FD (kid=True: KID) in DINOv2 space

The network, per image:

1. ``F.interpolate(mode='bicubic', align_corners=False)`` to size x size (the rule of rick_amd/clip.py: A = -0.75, clamped
   source indices, no antialiasing, overshoot kept), then ``(x * 0.5 + 0.5 - mean_c) / std_c`` with ImageNet's mean and std.
   This is NOT the PIL preprocessing of the DINOv2 evaluation scripts (antialiased bicubic on uint8): it is the differentiable-
   pipeline form on the generator's fp32 output, as for CLIP.
2. a P x P stride-P convolution WITH bias -> G x G patches of width Wd in row-major order;
3. tokens = [cls_token ; patches] + position_embeddings [T, Wd], T = G^2 + 1.  There is no LayerNorm in front of the blocks;
4. L blocks: t += ls1 * out(attn(norm1(t))); t += ls2 * fc2(gelu(fc1(norm2(t)))), gelu(u) = 0.5 u (1 + erf(u / sqrt 2)) (the
   exact one), ls1 and ls2 the LayerScale vectors [Wd], LayerNorm eps 1e-6; attention as in CLIP's tower;
5. the final LayerNorm on token 0 -> [N, Wd].  No projection.

The positional embedding is interpolated once at load, on the host, from the checkpoint's grid to (size / P)^2 by the rule of
transformers' ``Dinov2Embeddings.interpolate_pos_encoding``: the class row is kept, the patch rows are reshaped to
[1, Wd, g, g] and resized with ``F.interpolate(size=, mode='bicubic', align_corners=False)`` in fp32; nothing is done when the
grids agree.

CUDA fp32 inputs run rick_vit_input_f32, rick_inc_conv_lin_f32 (patch embedding, q/k/v), rick_vit_tokens_f32,
rick_clip_layernorm_f32, rick_clip_attention_f32 and rick_inc_conv_vit_f32 (out, fc1 + GELU, fc2, the last two with the
LayerScale and the residual in the epilogue): include/rick_hip.h "DINOv2".  The blocks are CLIP's (rick_amd/cliptower.py)
with other data.  An image's features are bit-identical whatever batch it is computed in.  The workspace for ``batch`` images
and every packed operand are allocated once at construction; a call allocates its output only and has no host branch on
data, so it can be captured in a hipGraph.  CPU tensors run the same network as a plain fp32 torch composition.

``src`` is a state_dict in one of two layouts, cast to fp32:

* transformers (``Dinov2Model``, with or without the ``dinov2.`` prefix of the task heads):
  ``embeddings.{cls_token [1, 1, Wd], position_embeddings [1, T, Wd], patch_embeddings.projection.{weight,bias}}``,
  ``encoder.layer.{i}.{norm1, attention.attention.{query,key,value}, attention.output.dense, layer_scale1.lambda1, norm2,
  mlp.fc1, mlp.fc2, layer_scale2.lambda1}``, ``layernorm.{weight,bias}``; ``embeddings.mask_token`` and ``classifier.*`` are
  ignored;
* the original release's: ``cls_token``, ``pos_embed``, ``patch_embed.proj.*``, ``blocks.{i}.{norm1, attn.qkv, attn.proj,
  ls1.gamma, norm2, mlp.fc1, mlp.fc2, ls2.gamma}``, ``norm.*``; ``mask_token`` is ignored.  (Recalled, not verified: PAPERS.md.)

Refused, with the key in the message: ``register_tokens`` (the models "with registers" have 261 tokens at 224 px), the SwiGLU
MLP of the giant model (``mlp.weights_in`` / ``mlp.w12``) and any other unknown key.  The configuration is read from the
shapes; heads = Wd / 64 unless ``heads`` is given.  Supported: size a multiple of P, (size / P)^2 + 1 <= 257 (ViT-*/14 at
224), a square checkpoint grid, head dim in {16, 32, 64}, Wd and the MLP width multiples of 4, Wd <= 2048.
"""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import gemm_conv
from .cliptower import (ATTENTION, Transformer, blocks_from_state_dict, column_block, gemm, issue, launch, limits, operand,
                        refuse_unexpected, shape, torch_blocks)
from .netutil import check_images, cuda_device, get, load_dict

WHO = 'Dinov2Features'
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
EPS = 1e-6

Dinov2Config = namedtuple('Dinov2Config', 'width patch tokens grid size layers mlp dim heads')       # dim = width: no projection

# ---- loading --------------------------------------------------------------------------------------------------------------
_get = functools.partial(get, who=WHO, errors=(RuntimeError, RuntimeError))
_BLOCK_HF = {'ln1': 'norm1', 'qkv': ('attention.attention.query', 'attention.attention.key', 'attention.attention.value'),
             'out': 'attention.output.dense', 'ln2': 'norm2', 'fc': 'mlp.fc1', 'proj': 'mlp.fc2', 'ls1': 'layer_scale1.lambda1',
             'ls2': 'layer_scale2.lambda1'}
_BLOCK_ORIGINAL = {'ln1': 'norm1', 'qkv': ('attn.qkv.weight', 'attn.qkv.bias'), 'out': 'attn.proj', 'ln2': 'norm2', 'fc': 'mlp.fc1',
                   'proj': 'mlp.fc2', 'ls1': 'ls1.gamma', 'ls2': 'ls2.gamma'}
_SWIGLU = ('mlp.weights_in', 'mlp.weights_out', 'mlp.w12', 'mlp.w3')


def params_from_state_dict(sd):
    """Either layout -> the network's parameters as fp32 CPU tensors under layout-free names: conv1 [Wd, 3, P, P], conv1.b
    [Wd], cls [Wd], pos [T, Wd] (the checkpoint's grid), blocks.{i}.{ln1.{w,b}, qkv.{w [3 Wd, Wd], b}, out.{w,b}, ls1 [Wd],
    ln2.{w,b}, fc.{w [M, Wd], b}, proj.{w [Wd, M], b}, ls2 [Wd]}, ln_post.{w,b}."""
    for k in sd:
        if 'register_tokens' in k:
            raise RuntimeError(f'{WHO}: key {k!r}: the models with registers are not supported (261 tokens at 224 px)')
        if any(s in k for s in _SWIGLU):
            raise RuntimeError(f'{WHO}: key {k!r}: the SwiGLU MLP (the giant model) is not supported')
    v = 'dinov2.' if any(k.startswith('dinov2.') for k in sd) else ''
    hf = any(k.startswith((v + 'embeddings.', v + 'encoder.layer.')) for k in sd)
    if hf:
        emb, pre, block = v + 'embeddings.', v + 'encoder.layer.', _BLOCK_HF
        k_conv, k_cls, k_pos, k_ln = emb + 'patch_embeddings.projection', emb + 'cls_token', emb + 'position_embeddings', v + 'layernorm'
        ignored = lambda k: k == emb + 'mask_token' or k.startswith('classifier.')            # noqa: E731
    else:
        pre, block = 'blocks.', _BLOCK_ORIGINAL
        k_conv, k_cls, k_pos, k_ln = 'patch_embed.proj', 'cls_token', 'pos_embed', 'norm'
        ignored = lambda k: k == 'mask_token'                                                  # noqa: E731
    cshape = shape(sd, k_conv + '.weight', WHO)
    if len(cshape) != 4 or cshape[1] != 3 or cshape[2] != cshape[3]:
        raise RuntimeError(f'{WHO}: key {k_conv + ".weight"!r} has shape {cshape}, expected (Wd, 3, P, P)')
    wd = cshape[0]
    pshape = shape(sd, k_pos, WHO)
    if len(pshape) != 3 or pshape[0] != 1 or pshape[2] != wd:
        raise RuntimeError(f'{WHO}: key {k_pos!r} has shape {pshape}, expected (1, T, {wd})')
    grid = math.isqrt(max(pshape[1] - 1, 0))
    if pshape[1] < 2 or grid * grid + 1 != pshape[1]:
        raise RuntimeError(f'{WHO}: key {k_pos!r} has {pshape[1]} rows, expected G^2 + 1 (a square grid and the class row)')
    p = {'conv1': _get(sd, k_conv + '.weight', cshape), 'conv1.b': _get(sd, k_conv + '.bias', (wd,)),
         'cls': _get(sd, k_cls, (1, 1, wd)).reshape(wd), 'pos': _get(sd, k_pos, pshape).reshape(pshape[1], wd)}
    used = {k_conv + '.weight', k_conv + '.bias', k_cls, k_pos}
    for s, suffix in (('w', 'weight'), ('b', 'bias')):
        p[f'ln_post.{s}'] = _get(sd, f'{k_ln}.{suffix}', (wd,))
        used.add(f'{k_ln}.{suffix}')
    blocks, keys = blocks_from_state_dict(sd, pre, hf, wd, WHO, block)
    p.update(blocks)
    refuse_unexpected(sd, used | keys, ignored, WHO)
    return p


def interpolate_pos(pos, grid):
    """pos [g^2 + 1, Wd] -> [grid^2 + 1, Wd] by the rule in the module docstring; pos itself when g == grid."""
    g, wd = math.isqrt(pos.shape[0] - 1), pos.shape[1]
    if g == grid:
        return pos
    patch = F.interpolate(pos[1:].reshape(1, g, g, wd).permute(0, 3, 1, 2).float(), size=(grid, grid), mode='bicubic', align_corners=False)
    return torch.cat([pos[:1], patch.permute(0, 2, 3, 1).reshape(grid * grid, wd).to(pos.dtype)]).contiguous()


def config_from_params(p, size, heads=None):
    """The configuration the shapes and the image size imply; refuses what the kernels do not support."""
    wd, _, patch, _ = p['conv1'].shape
    if size < patch or size % patch:
        raise RuntimeError(f'{WHO}: size {size} is no multiple of the patch size {patch}')
    grid = size // patch
    layers, mlp, heads = limits(p, wd, grid * grid + 1, heads, f'tokens per image at size {size}', WHO)
    return Dinov2Config(wd, patch, grid * grid + 1, grid, size, layers, mlp, wd, heads)


# ---- the network as a plain torch composition -----------------------------------------------------------------------------
def resize_affine(x, size):
    """Step 1: x [N, 3, H, W] in [-1, 1] -> [N, 3, size, size], bicubic resize and ImageNet's affine."""
    x = F.interpolate(x, size=(size, size), mode='bicubic', align_corners=False)
    mean, std = (torch.tensor(v, dtype=x.dtype, device=x.device).view(1, 3, 1, 1) for v in (MEAN, STD))
    return (x * 0.5 + 0.5 - mean) / std


def torch_forward(p, cfg, x):
    """The whole network on x [N, 3, H, W] in the dtype and on the device of x and the parameters p (pos at cfg's grid) ->
    [N, Wd]."""
    wd = cfg.width
    t = F.conv2d(resize_affine(x, cfg.size), p['conv1'], p['conv1.b'], stride=cfg.patch).flatten(2).transpose(1, 2)
    t = torch.cat([p['cls'].expand(t.shape[0], 1, wd), t], 1) + p['pos']
    t = torch_blocks(p, cfg, t, eps=EPS, act='gelu')
    return F.layer_norm(t[:, 0], (wd,), p['ln_post.w'], p['ln_post.b'], EPS)


# ---- device plan ----------------------------------------------------------------------------------------------------------
def pack_patch_embedding(w, b, bn=None):
    """conv1 [Wd, 3, P, P] and its bias -> the operand of the P x P stride-P convolution on the NHWC4 input: rows (ky, kx, c)
    with c < 4 and a zero row for c = 3.  (wpk, bias, Cop, bn)."""
    return gemm_conv.pack(w, b, ci_pad=4, bn=bn)


class _Plan:
    """Packed operands and the workspace of `batch` images on the device: the NHWC4 input, the patch rows and the transformer's
    buffers (rick_amd/cliptower.py), without a projection."""

    def __init__(self, p, cfg, batch, device):
        self.cfg, self.batch, self.fwd = cfg, batch, {}
        self.patch = operand(pack_patch_embedding(p['conv1'], p['conv1.b'], column_block(cfg.width, batch * (cfg.tokens - 1))), device)
        self.tf = Transformer(p, cfg, batch, device, WHO, ATTENTION, eps=EPS, act='gelu', head=False,
                              stem=(batch * cfg.size * cfg.size * 4, batch * (cfg.tokens - 1) * cfg.width))
        self.x0, self.patches = self.tf.stem

    def run(self, x, out):
        """x [n, 3, H, W] fp32 contiguous, n <= batch -> out [n, Wd] (contiguous rows).  Everything but the input kernel, which
        reads x, and the final LayerNorm, which writes out, is resolved once per n."""
        from . import _lib as L
        c, tf = self.cfg, self.tf
        n, _, H, W = x.shape
        if n not in self.fwd:
            v, P = tf.vec, (c.patch, c.patch)
            _, _, cop, bn = self.patch
            a = gemm_conv.descriptor(n, c.size, c.size, 4, P, P, (0, 0), cop, bn, [(self.patches.data_ptr(), c.width, 0, c.width)])
            self.fwd[n] = [gemm('patch', self.patch, a, self.x0),
                           launch('tokens', 'rick_vit_tokens_f32', self.patches.data_ptr(), v['cls'].data_ptr(), v['pos'].data_ptr(),
                                  tf.res[0].data_ptr(), n, c.tokens, c.width),
                           *tf.launches(n)]
        stream = L.stream_ptr()
        L.check(L.lib.rick_vit_input_f32(x.data_ptr(), self.x0.data_ptr(), n, H, W, c.size, *MEAN, *STD, stream), 'rick_vit_input_f32')
        issue(self.fwd[n], stream)
        issue([tf.layernorm('ln_post', 'ln_post', tf.res[-1], c.tokens * c.width, out, n)], stream)      # token 0 of every image


class Dinov2Features:
    """DINOv2's ViT up to the final LayerNorm's class token on HIP kernels; see the module docstring."""

    def __init__(self, params, device='cuda', batch=25, size=224, heads=None):
        if batch < 1:
            raise ValueError(f'{WHO}: batch must be >= 1')
        self.cfg = config_from_params(params, int(size), heads)
        self.params = {**params, 'pos': interpolate_pos(params['pos'], self.cfg.grid)}
        self.batch = int(batch)
        self.device = cuda_device(device)
        self._plan = None
        if self.device.type == 'cuda':
            with torch.cuda.device(self.device):
                self._plan = _Plan(self.params, self.cfg, self.batch, self.device)

    @classmethod
    def load(cls, src, device='cuda', batch=25, size=224, heads=None):
        """src: a path or state_dict in the transformers or the original layout; size: the side the images are resized to."""
        return cls(params_from_state_dict(load_dict(src)), device=device, batch=batch, size=size, heads=heads)

    @torch.no_grad()
    def __call__(self, x):
        """x [N, 3, H, W] fp32 in [-1, 1] -> the normalised class tokens [N, Wd] fp32 on x's device."""
        check_images(x, WHO, self.device)
        N = x.shape[0]
        if x.device.type == 'cpu':
            out = torch.empty((N, self.cfg.width), dtype=torch.float32)
            for lo in range(0, N, self.batch):
                out[lo:lo + self.batch] = torch_forward(self.params, self.cfg, x[lo:lo + self.batch])
            return out
        out = torch.empty((N, self.cfg.width), device=x.device, dtype=torch.float32)
        x = x.contiguous()
        with torch.cuda.device(self.device):
            for lo in range(0, N, self.batch):
                hi = min(N, lo + self.batch)
                self._plan.run(x[lo:hi], out[lo:hi])
        return out
