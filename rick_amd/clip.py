"""CLIP's ViT image tower (Radford et al., 2021) on HIP kernels: the unnormalised image embeddings that ``encode_image``
returns, for FID / KID in CLIP space, and their gradient with respect to the image for the CLIP-guided adaptation losses
(rick_amd/clipguide.py).  The weights are frozen: there are no weight gradients.

    net = ClipImageFeatures.load(src, device='cuda', batch=25)       # src: a state_dict or a path, either layout below
    f = net(x)                                  # x [N, 3, H, W] fp32 in [-1, 1] -> [N, D] fp32 on x's device
    ev = Evaluator(g_ema, net, net(real_images))                     # FID (kid=True: KID) in CLIP space
    sim = clip_similarity(net(a), net(b))                            # rick_amd/evaluate.py
    e = net.encode(x)                           # the same bits; differentiable (first order) with respect to x

``encode`` keeps, per layer, what the backward pass reads (the residual stream before ln_1 and ln_2, q|k|v, the c_fc
pre-activation) and runs the adjoint of every stage on HIP kernels: rick_clip_input_bwd_f32, rick_clip_tokens_bwd_f32,
rick_clip_layernorm_bwd_f32, rick_clip_attention_bwd_f32, rick_clip_quickgelu_bwd_f32, the five data-gradient GEMMs of a
layer on rick_inc_conv_lin_f32 over transposed operands, and the projection's on rick_fc_f32.  ``prepare_grad`` sizes that
workspace; ``__call__`` is untouched by it.

The network, per image:

1. ``F.interpolate(mode='bicubic', align_corners=False)`` to S x S (A = -0.75, clamped source indices, no antialiasing,
   overshoot kept), then ``(x * 0.5 + 0.5 - mean_c) / std_c`` with CLIP's mean and std.  This is NOT CLIP's PIL preprocessing
   (antialiased bicubic on uint8 with rounding): it is the differentiable-pipeline form, applied to the generator's fp32
   output.  At H == W == S the resize copies the values.
2. a P x P stride-P convolution without bias -> G x G patches of width Wd in row-major order;
   tokens = [class_embedding ; patches] + positional_embedding [T, Wd], T = G^2 + 1;
3. ``ln_pre`` (LayerNorm over Wd, eps 1e-5, biased variance);
4. L blocks: t += out_proj(attn(ln_1(t))); t += c_proj(quickgelu(c_fc(ln_2(t)))), quickgelu(u) = u sigmoid(1.702 u);
   attention per head h on columns [h d, (h + 1) d): softmax(q k^T / sqrt(d)) v;
5. ``ln_post`` on token 0, then the projection without bias -> [N, D].

CUDA fp32 inputs run rick_clip_input_f32, rick_inc_conv_lin_f32 (the f32 implicit GEMM with the linear / QuickGELU / residual
epilogue: patch embedding, the fused q/k/v projection, out_proj, c_fc, c_proj), rick_clip_tokens_f32, rick_clip_layernorm_f32,
rick_clip_attention_f32 and rick_fc_f32 for the projection (include/rick_hip.h "CLIP").  An image's embedding is
bit-identical whatever batch it is computed in.  The workspace for ``batch`` images and every packed operand are allocated
once at construction; a call allocates its output only and has no host branch on data, so it can be captured in a hipGraph.
CPU tensors run the same network as a plain fp32 torch composition (``torch_forward``).

``src`` is a state_dict in one of two layouts, cast to fp32 (OpenAI checkpoints are fp16):

* transformers (``CLIPModel`` / ``CLIPVisionModelWithProjection``): ``vision_model.embeddings.{class_embedding,
  patch_embedding.weight, position_embedding.weight}``, ``vision_model.pre_layrnorm.*`` (the library's spelling),
  ``vision_model.encoder.layers.{i}.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.fc1, mlp.fc2}.*``,
  ``vision_model.post_layernorm.*``, ``visual_projection.weight [D, Wd]``;
* OpenAI, with or without the ``visual.`` prefix: ``conv1.weight``, ``class_embedding``, ``positional_embedding``,
  ``ln_pre.*``, ``transformer.resblocks.{i}.{ln_1.*, attn.in_proj_weight [3 Wd, Wd] (rows q, k, v), attn.in_proj_bias,
  attn.out_proj.*, ln_2.*, mlp.c_fc.*, mlp.c_proj.*}``, ``ln_post.*``, ``proj [Wd, D]``.

Text-tower keys, ``logit_scale`` and ``position_ids`` are ignored; any other unknown key raises.  The configuration is read
from the shapes; heads = Wd / 64 (CLIP's rule) unless ``heads`` is given.  Supported: head dim in {16, 32, 64}, T <= 257
(ViT-L/14 at 224), Wd and the MLP width multiples of 4, Wd <= 2048.
"""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import gemm_conv
from .fc import FC_MAX_ROWS, check_packed, pack_fc_weight, run_fc
from .netutil import check_images, cuda_device, get, load_dict

WHO = 'ClipImageFeatures'
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
EPS = 1e-5
MAX_TOKENS, MAX_WIDTH, HEAD_DIMS = 257, 2048, (16, 32, 64)
CUS = 256                       # compute units of the MI355X

ClipConfig = namedtuple('ClipConfig', 'width patch tokens grid size layers mlp dim heads')

# ---- loading --------------------------------------------------------------------------------------------------------------
_get = functools.partial(get, who=WHO, errors=(RuntimeError, RuntimeError))
_OPENAI_TEXT = ('token_embedding.', 'ln_final.', 'text_projection', 'logit_scale', 'input_resolution', 'context_length', 'vocab_size')
_BLOCK_OPENAI = {'ln1': 'ln_1', 'out': 'attn.out_proj', 'ln2': 'ln_2', 'fc': 'mlp.c_fc', 'proj': 'mlp.c_proj'}
_BLOCK_HF = {'ln1': 'layer_norm1', 'out': 'self_attn.out_proj', 'ln2': 'layer_norm2', 'fc': 'mlp.fc1', 'proj': 'mlp.fc2'}


def _shape(sd, key):
    if key not in sd:
        raise RuntimeError(f'{WHO}: missing key {key!r}')
    return tuple(torch.as_tensor(sd[key]).shape)


def _layer_count(keys, prefix):
    idx = [int(k[len(prefix):].split('.')[0]) for k in keys if k.startswith(prefix) and k[len(prefix):].split('.')[0].isdigit()]
    if not idx:
        raise RuntimeError(f'{WHO}: missing key {prefix + "0"!r}...: no transformer layer in the state_dict')
    return max(idx) + 1


def params_from_state_dict(sd):
    """Either layout -> the network's parameters as fp32 CPU tensors under layout-free names: conv1 [Wd, 3, P, P], cls [Wd],
    pos [T, Wd], ln_pre.{w,b}, blocks.{i}.{ln1.{w,b}, qkv.{w [3 Wd, Wd], b}, out.{w,b}, ln2.{w,b}, fc.{w [M, Wd], b},
    proj.{w [Wd, M], b}}, ln_post.{w,b}, head [D, Wd]."""
    hf = any(k.startswith('vision_model.') for k in sd)
    used, p = set(), {}

    def take(name, key, shape):
        p[name] = _get(sd, key, shape)
        used.add(key)

    if hf:
        emb, pre, wb = 'vision_model.embeddings.', 'vision_model.encoder.layers.', (('w', 'weight'), ('b', 'bias'))
        k_conv, k_cls, k_pos = emb + 'patch_embedding.weight', emb + 'class_embedding', emb + 'position_embedding.weight'
        k_lnpre, k_lnpost, k_head = 'vision_model.pre_layrnorm', 'vision_model.post_layernorm', 'visual_projection.weight'
        block = _BLOCK_HF
        ignored = lambda k: (k.startswith('text_model.') or k in ('text_projection.weight', 'logit_scale')      # noqa: E731
                             or k.endswith('position_ids'))
    else:
        v = 'visual.' if 'visual.conv1.weight' in sd else ''
        pre, wb = v + 'transformer.resblocks.', (('w', 'weight'), ('b', 'bias'))
        k_conv, k_cls, k_pos = v + 'conv1.weight', v + 'class_embedding', v + 'positional_embedding'
        k_lnpre, k_lnpost, k_head = v + 'ln_pre', v + 'ln_post', v + 'proj'
        block = _BLOCK_OPENAI
        # beside a prefixed image tower, the unprefixed transformer and positional embedding are the text tower's
        ignored = lambda k: (k.startswith(_OPENAI_TEXT) or k.endswith('position_ids')                           # noqa: E731
                             or (v and (k.startswith('transformer.') or k == 'positional_embedding')))
    cshape = _shape(sd, k_conv)
    if len(cshape) != 4 or cshape[1] != 3 or cshape[2] != cshape[3]:
        raise RuntimeError(f'{WHO}: key {k_conv!r} has shape {cshape}, expected (Wd, 3, P, P)')
    wd = cshape[0]
    pshape = _shape(sd, k_pos)
    take('conv1', k_conv, cshape)
    take('cls', k_cls, (wd,))
    take('pos', k_pos, (pshape[0], wd) if len(pshape) == 2 else (0, wd))
    for name, key in (('ln_pre', k_lnpre), ('ln_post', k_lnpost)):
        for s, suffix in wb:
            take(f'{name}.{s}', f'{key}.{suffix}', (wd,))
    layers = _layer_count(sd.keys(), pre)
    for i in range(layers):
        src, dst = f'{pre}{i}.', f'blocks.{i}.'
        mlp = _shape(sd, f'{src}{block["fc"]}.weight')[0]
        if hf:
            parts = []
            for s, suffix in wb:
                for proj in 'qkv':
                    key = f'{src}self_attn.{proj}_proj.{suffix}'
                    parts.append(_get(sd, key, (wd, wd) if s == 'w' else (wd,)))
                    used.add(key)
            p[dst + 'qkv.w'], p[dst + 'qkv.b'] = torch.cat(parts[:3]).contiguous(), torch.cat(parts[3:]).contiguous()
        else:
            take(dst + 'qkv.w', src + 'attn.in_proj_weight', (3 * wd, wd))
            take(dst + 'qkv.b', src + 'attn.in_proj_bias', (3 * wd,))
        for name, shape in (('ln1', None), ('out', (wd, wd)), ('ln2', None), ('fc', (mlp, wd)), ('proj', (wd, mlp))):
            take(f'{dst}{name}.w', f'{src}{block[name]}.weight', shape or (wd,))
            take(f'{dst}{name}.b', f'{src}{block[name]}.bias', (shape[0],) if shape else (wd,))
    hshape = _shape(sd, k_head)
    if len(hshape) != 2 or hshape[1 if hf else 0] != wd:
        raise RuntimeError(f'{WHO}: key {k_head!r} has shape {hshape}, expected {"(D, Wd)" if hf else "(Wd, D)"}')
    take('head', k_head, hshape)
    if not hf:
        p['head'] = p['head'].t().contiguous()                # OpenAI's proj is [Wd, D]
    extra = sorted(k for k in sd if k not in used and not ignored(k))
    if extra:
        raise RuntimeError(f'{WHO}: unexpected key {extra[0]!r} in the state_dict')
    return p


def config_from_params(p, heads=None):
    """The configuration the shapes imply; refuses what the kernels do not support."""
    wd, _, patch, _ = p['conv1'].shape
    tokens = p['pos'].shape[0]
    grid = math.isqrt(max(tokens - 1, 0))
    if tokens > MAX_TOKENS:
        raise RuntimeError(f'{WHO}: {tokens} tokens per image, at most {MAX_TOKENS} are supported')
    if tokens < 2 or grid * grid + 1 != tokens:
        raise RuntimeError(f'{WHO}: positional embedding has {tokens} rows, expected G^2 + 1')
    layers = 1 + max(int(k.split('.')[1]) for k in p if k.startswith('blocks.'))
    mlp = p['blocks.0.fc.w'].shape[0]
    if wd % 4 or mlp % 4 or wd > MAX_WIDTH:
        raise RuntimeError(f'{WHO}: width {wd} / MLP width {mlp}: multiples of 4 and a width of at most {MAX_WIDTH} are supported')
    if heads is None:
        if wd % 64:
            raise RuntimeError(f'{WHO}: width {wd} is no multiple of 64 (heads = width / 64 is CLIP\'s rule); pass heads=')
        heads = wd // 64
    if heads < 1 or wd % heads or wd // heads not in HEAD_DIMS:
        raise RuntimeError(f'{WHO}: width {wd} with {heads} heads: the head dim must be one of {HEAD_DIMS}')
    return ClipConfig(wd, patch, tokens, grid, grid * patch, layers, mlp, p['head'].shape[0], int(heads))


# ---- the network as a plain torch composition -----------------------------------------------------------------------------
def resize_affine(x, size):
    """Step 1: x [N, 3, H, W] in [-1, 1] -> [N, 3, size, size], bicubic resize and CLIP's affine."""
    x = F.interpolate(x, size=(size, size), mode='bicubic', align_corners=False)
    mean, std = (torch.tensor(v, dtype=x.dtype, device=x.device).view(1, 3, 1, 1) for v in (MEAN, STD))
    return (x * 0.5 + 0.5 - mean) / std


def torch_forward(p, cfg, x):
    """The whole network on x [N, 3, H, W] in the dtype and on the device of x and the parameters p -> [N, D]."""
    return torch_tower(p, cfg, F.conv2d(resize_affine(x, cfg.size), p['conv1'], stride=cfg.patch).flatten(2).transpose(1, 2))


def torch_tower(p, cfg, t):
    """Steps 2 (from the patch rows t [n, G^2, Wd] on) to 5 of the network -> [n, D]."""
    wd, d = cfg.width, cfg.width // cfg.heads
    n = t.shape[0]
    t = torch.cat([p['cls'].expand(n, 1, wd), t], 1) + p['pos']
    t = F.layer_norm(t, (wd,), p['ln_pre.w'], p['ln_pre.b'], EPS)
    for i in range(cfg.layers):
        b = f'blocks.{i}.'
        h = F.layer_norm(t, (wd,), p[b + 'ln1.w'], p[b + 'ln1.b'], EPS)
        q, k, v = (u.view(n, cfg.tokens, cfg.heads, d).transpose(1, 2) for u in F.linear(h, p[b + 'qkv.w'], p[b + 'qkv.b']).split(wd, 2))
        a = torch.softmax(q @ k.transpose(2, 3) * (1.0 / math.sqrt(d)), -1) @ v
        t = t + F.linear(a.transpose(1, 2).reshape(n, cfg.tokens, wd), p[b + 'out.w'], p[b + 'out.b'])
        h = F.linear(F.layer_norm(t, (wd,), p[b + 'ln2.w'], p[b + 'ln2.b'], EPS), p[b + 'fc.w'], p[b + 'fc.b'])
        t = t + F.linear(h * torch.sigmoid(1.702 * h), p[b + 'proj.w'], p[b + 'proj.b'])
    return F.linear(F.layer_norm(t[:, 0], (wd,), p['ln_post.w'], p['ln_post.b'], EPS), p['head'])


# ---- GEMM operands --------------------------------------------------------------------------------------------------------
def pack_patch_embedding(w, bn=None):
    """conv1 [Wd, 3, P, P] -> the operand of the P x P stride-P convolution on the NHWC4 input: rows (ky, kx, c) with c < 4 and
    a zero row for c = 3.  No bias.  (wpk, bias, Cop, bn)."""
    return gemm_conv.pack(w, None, ci_pad=4, bn=bn)


def pack_linear(w, b, bn=None):
    """A linear layer W [out, in], b [out] as the 1 x 1 convolution's operand: wpk[k, o] = W[o, k].  (wpk, bias, Cop, bn)."""
    return gemm_conv.pack(w[:, :, None, None], b, bn=bn)


def pack_linear_transposed(w, bn=None):
    """The data gradient of a linear layer W [out, in] as a linear layer of its own: gx = gy W, so the operand is pack_linear's
    of W^T [in, out] with a zero bias, wpk[o, k] = W[o, k].  (wpk, zero bias, Cop, bn)."""
    return gemm_conv.pack(w.t()[:, :, None, None], None, bn=bn)


def pack_patch_embedding_transposed(w, bn=None):
    """The data gradient of the patch embedding: patch rows [N G^2, Wd] -> [N G^2, 4 P^2] in pack_patch_embedding's row order
    (ky, kx, c4), a linear layer whose weight is that operand transposed (the rows of c = 3 are zero)."""
    wd, _, p, _ = w.shape
    rows = F.pad(w, (0, 0, 0, 0, 0, 1)).permute(2, 3, 1, 0).reshape(4 * p * p, wd)
    return gemm_conv.pack(rows[:, :, None, None], None, bn=bn)


def column_block(co, rows):
    """gemm_conv.column_block(co), but 64 where 128-column blocks on `rows` GEMM rows (a full batch) would leave some of the
    256 CUs without a block: the kernel's tiles are 128 rows tall, there is no split-K, and a block's time is set by K.  The
    sums, and so the bits, do not depend on the block."""
    bn = gemm_conv.column_block(co)
    return 64 if bn == 128 and -(-rows // 128) * (co // 128) < CUS else bn


# ---- device plan ----------------------------------------------------------------------------------------------------------
class _Plan:
    """Packed operands and the workspace of `batch` images on the device.

    Per image, in floats: the NHWC4 input 4 S^2, the patch rows G^2 Wd, and per token the residual stream Wd, the LayerNorm
    output Wd, q|k|v 3 Wd, the attention output Wd and the MLP's hidden layer: 2.5 MB per image at ViT-B/32, 62 MB at the default
    25, next to 0.35 GB of packed weights."""

    def __init__(self, p, cfg, batch, device):
        from . import _lib
        self._lib = _lib
        self.cfg, self.batch = cfg, batch
        f32 = dict(device=device, dtype=torch.float32)
        self.vec = {k: v.to(device) for k, v in p.items() if v.dim() == 1 or k == 'pos'}
        self.gemm = {}
        self._add_gemm('patch', pack_patch_embedding(p['conv1'], column_block(cfg.width, batch * (cfg.tokens - 1))), device)
        for i in range(cfg.layers):
            for name in ('qkv', 'out', 'fc', 'proj'):
                w = p[f'blocks.{i}.{name}.w']
                self._add_gemm(f'blocks.{i}.{name}', pack_linear(w, p[f'blocks.{i}.{name}.b'], column_block(w.shape[0], batch * cfg.tokens)),
                               device)
        head = pack_fc_weight(p['head'])
        check_packed(head, cfg.width, cfg.dim, WHO)
        self.head, self.head_bias = head.to(device), torch.zeros(cfg.dim, **f32)
        rows = batch * cfg.tokens
        self.x0 = torch.empty(batch * cfg.size * cfg.size * 4, **f32)
        self.patches = torch.empty(batch * (cfg.tokens - 1) * cfg.width, **f32)
        self.tok, self.ln, self.att = (torch.empty(rows * cfg.width, **f32) for _ in range(3))
        self.qkv = torch.empty(rows * 3 * cfg.width, **f32)
        self.hid = torch.empty(rows * cfg.mlp, **f32)
        self.post = torch.empty(batch * cfg.width, **f32)
        self.ws = torch.empty(_lib.lib.rick_fc_workspace_floats(min(batch, FC_MAX_ROWS), cfg.width, cfg.dim), **f32)
        self._desc = {}

    def _add_gemm(self, name, packed, device):
        wpk, bias, cop, bn = packed
        self.gemm[name] = (wpk.to(device), bias.to(device), cop, bn)

    def _descriptors(self, n):
        """The rick_inc_conv of every GEMM for n images (host structures, built once per n)."""
        if n not in self._desc:
            c, d = self.cfg, {}
            rows = n * c.tokens

            def lin(name, k, co, dst):
                _, _, cop, bn = self.gemm[name]
                return gemm_conv.descriptor(rows, 1, 1, k, (1, 1), (1, 1), (0, 0), cop, bn, [(dst.data_ptr(), co, 0, co)])

            _, _, cop, bn = self.gemm['patch']
            d['patch'] = gemm_conv.descriptor(n, c.size, c.size, 4, (c.patch, c.patch), (c.patch, c.patch), (0, 0), cop, bn,
                                              [(self.patches.data_ptr(), c.width, 0, c.width)])
            for i in range(c.layers):
                b = f'blocks.{i}.'
                d[b + 'qkv'] = lin(b + 'qkv', c.width, 3 * c.width, self.qkv)
                d[b + 'out'] = lin(b + 'out', c.width, c.width, self.tok)
                d[b + 'fc'] = lin(b + 'fc', c.width, c.mlp, self.hid)
                d[b + 'proj'] = lin(b + 'proj', c.mlp, c.width, self.tok)
            self._desc[n] = d
        return self._desc[n]

    def run(self, x, out):
        """x [n, 3, H, W] fp32 contiguous, n <= batch -> out [n, D] (contiguous rows)."""
        L, c = self._lib, self.cfg
        lib, stream = L.lib, L.stream_ptr()
        n, _, H, W = x.shape
        rows, d, v = n * c.tokens, self._descriptors(n), self.vec

        def gemm(name, src, res=None, act=0):
            wpk, bias, _, _ = self.gemm[name]
            L.check(lib.rick_inc_conv_lin_f32(src.data_ptr(), wpk.data_ptr(), bias.data_ptr(), None if res is None else res.data_ptr(),
                                              act, d[name], stream), 'rick_inc_conv_lin_f32')

        def layernorm(name, src, ldx, dst, r):
            L.check(lib.rick_clip_layernorm_f32(src.data_ptr(), ldx, v[name + '.w'].data_ptr(), v[name + '.b'].data_ptr(), dst.data_ptr(),
                                                r, c.width, EPS, stream), 'rick_clip_layernorm_f32')

        L.check(lib.rick_clip_input_f32(x.data_ptr(), self.x0.data_ptr(), n, H, W, c.size, stream), 'rick_clip_input_f32')
        gemm('patch', self.x0)
        L.check(lib.rick_clip_tokens_f32(self.patches.data_ptr(), v['cls'].data_ptr(), v['pos'].data_ptr(), v['ln_pre.w'].data_ptr(),
                                         v['ln_pre.b'].data_ptr(), self.tok.data_ptr(), n, c.tokens, c.width, EPS, stream),
                'rick_clip_tokens_f32')
        for i in range(c.layers):
            b = f'blocks.{i}.'
            layernorm(b + 'ln1', self.tok, c.width, self.ln, rows)
            gemm(b + 'qkv', self.ln)
            L.check(lib.rick_clip_attention_f32(self.qkv.data_ptr(), self.att.data_ptr(), n, c.tokens, c.heads, c.width // c.heads,
                                                stream), 'rick_clip_attention_f32')
            gemm(b + 'out', self.att, res=self.tok)           # the residual in place
            layernorm(b + 'ln2', self.tok, c.width, self.ln, rows)
            gemm(b + 'fc', self.ln, act=1)
            gemm(b + 'proj', self.hid, res=self.tok)
        layernorm('ln_post', self.tok, c.tokens * c.width, self.post, n)      # token 0 of every image
        run_fc(self.post.data_ptr(), self.head.data_ptr(), self.head_bias.data_ptr(), self.ws.data_ptr(), out.data_ptr(), n, c.width,
               c.dim, 0)


class _GradWorkspace:
    """What a differentiable call (``ClipImageFeatures.encode``) needs beyond the forward plan, for `batch` images.

    The transposed operands of the five GEMMs per layer and of the projection, packed once: about as much memory again as the
    forward operands (0.35 GB at ViT-B/32).  The activations the backward pass reads, kept per layer: the residual stream
    before ln_1 and before ln_2 (the residual GEMMs write a separate destination here instead of updating in place), q|k|v
    and the c_fc pre-activation (c_fc runs with the identity epilogue, rick_clip_quickgelu_f32 follows: the same bits as the
    fused epilogue), plus the patch rows: about 17 MB per image at ViT-B/32.  And the gradient buffers.  The forward scratch
    (LayerNorm output, attention output, the activated hidden layer) is the plan's.  `version` counts forward runs: a backward
    run whose activations were overwritten refuses."""

    def __init__(self, plan, p, batch, device):
        if batch < 1 or batch > plan.batch:
            raise ValueError(f'{WHO}: grad_batch must be between 1 and batch = {plan.batch}')
        self.plan, self.cfg, self.batch, self.version = plan, plan.cfg, int(batch), 0
        self._lib = plan._lib
        c, f32 = self.cfg, dict(device=device, dtype=torch.float32)
        rows = batch * c.tokens
        self.gemm = {}
        self._add('patch', pack_patch_embedding_transposed(p['conv1'], column_block(4 * c.patch * c.patch, batch * (c.tokens - 1))),
                  device)
        for i in range(c.layers):
            for name in ('qkv', 'out', 'fc', 'proj'):
                w = p[f'blocks.{i}.{name}.w']
                self._add(f'blocks.{i}.{name}', pack_linear_transposed(w, column_block(w.shape[1], rows)), device)
        head_t = pack_fc_weight(p['head'].t().contiguous())
        check_packed(head_t, c.dim, c.width, WHO)
        self.head_t, self.head_t_bias = head_t.to(device), torch.zeros(c.width, **f32)
        buf = lambda n: torch.empty(n, **f32)                                     # noqa: E731
        self.x0, self.patches = buf(batch * c.size * c.size * 4), buf(batch * (c.tokens - 1) * c.width)
        self.res = [buf(rows * c.width) for _ in range(2 * c.layers + 1)]
        self.qkv = [buf(rows * 3 * c.width) for _ in range(c.layers)]
        self.pre = [buf(rows * c.mlp) for _ in range(c.layers)]
        self.gt, self.ga, self.gh, self.gq = buf(rows * c.width), buf(rows * c.width), buf(rows * c.mlp), buf(rows * 3 * c.width)
        self.stats = buf(batch * c.heads * c.tokens * 3)
        self.gpost, self.gp, self.gx0 = buf(batch * c.width), buf(batch * (c.tokens - 1) * c.width), buf(batch * c.size * c.size * 4)
        self.ws = buf(self._lib.lib.rick_fc_workspace_floats(min(batch, FC_MAX_ROWS), c.dim, c.width))
        self._desc = {}

    def _add(self, name, packed, device):
        wpk, bias, cop, bn = packed
        self.gemm[name] = (wpk.to(device), bias.to(device), cop, bn)

    def _descriptors(self, n):
        """Forward ('f', name) and backward ('b', name) descriptors of every GEMM for n images, built once per n."""
        if n not in self._desc:
            c, pl, d = self.cfg, self.plan, {}
            rows = n * c.tokens

            def lin(table, name, k, co, dst):
                _, _, cop, bn = table[name]
                return gemm_conv.descriptor(rows, 1, 1, k, (1, 1), (1, 1), (0, 0), cop, bn, [(dst.data_ptr(), co, 0, co)])

            _, _, cop, bn = pl.gemm['patch']
            d['f', 'patch'] = gemm_conv.descriptor(n, c.size, c.size, 4, (c.patch, c.patch), (c.patch, c.patch), (0, 0), cop, bn,
                                                   [(self.patches.data_ptr(), c.width, 0, c.width)])
            _, _, cop, bn = self.gemm['patch']
            k2 = 4 * c.patch * c.patch
            d['b', 'patch'] = gemm_conv.descriptor(n * (c.tokens - 1), 1, 1, c.width, (1, 1), (1, 1), (0, 0), cop, bn,
                                                   [(self.gx0.data_ptr(), k2, 0, k2)])
            for i in range(c.layers):
                b = f'blocks.{i}.'
                d['f', b + 'qkv'] = lin(pl.gemm, b + 'qkv', c.width, 3 * c.width, self.qkv[i])
                d['f', b + 'out'] = lin(pl.gemm, b + 'out', c.width, c.width, self.res[2 * i + 1])
                d['f', b + 'fc'] = lin(pl.gemm, b + 'fc', c.width, c.mlp, self.pre[i])
                d['f', b + 'proj'] = lin(pl.gemm, b + 'proj', c.mlp, c.width, self.res[2 * i + 2])
                d['b', b + 'proj'] = lin(self.gemm, b + 'proj', c.width, c.mlp, self.gh)
                d['b', b + 'fc'] = lin(self.gemm, b + 'fc', c.mlp, c.width, self.ga)
                d['b', b + 'out'] = lin(self.gemm, b + 'out', c.width, c.width, self.ga)
                d['b', b + 'qkv'] = lin(self.gemm, b + 'qkv', 3 * c.width, c.width, self.ga)
            self._desc[n] = d
        return self._desc[n]

    def _gemm(self, table, desc, src, res=None):
        L = self._lib
        wpk, bias, _, _ = table
        L.check(L.lib.rick_inc_conv_lin_f32(src.data_ptr(), wpk.data_ptr(), bias.data_ptr(), None if res is None else res.data_ptr(), 0,
                                            desc, L.stream_ptr()), 'rick_inc_conv_lin_f32')

    def forward(self, x, out):
        """_Plan.run with the activations kept: x [n, 3, H, W] fp32 contiguous, n <= batch -> out [n, D], the same bits."""
        L, c, pl = self._lib, self.cfg, self.plan
        lib, stream = L.lib, L.stream_ptr()
        n, _, H, W = x.shape
        rows, d, v = n * c.tokens, self._descriptors(n), pl.vec
        self.version += 1

        def layernorm(name, src, ldx, dst, r):
            L.check(lib.rick_clip_layernorm_f32(src.data_ptr(), ldx, v[name + '.w'].data_ptr(), v[name + '.b'].data_ptr(), dst.data_ptr(),
                                                r, c.width, EPS, stream), 'rick_clip_layernorm_f32')

        L.check(lib.rick_clip_input_f32(x.data_ptr(), self.x0.data_ptr(), n, H, W, c.size, stream), 'rick_clip_input_f32')
        self._gemm(pl.gemm['patch'], d['f', 'patch'], self.x0)
        L.check(lib.rick_clip_tokens_f32(self.patches.data_ptr(), v['cls'].data_ptr(), v['pos'].data_ptr(), v['ln_pre.w'].data_ptr(),
                                         v['ln_pre.b'].data_ptr(), self.res[0].data_ptr(), n, c.tokens, c.width, EPS, stream),
                'rick_clip_tokens_f32')
        for i in range(c.layers):
            b = f'blocks.{i}.'
            t0, t1, t2 = self.res[2 * i:2 * i + 3]
            layernorm(b + 'ln1', t0, c.width, pl.ln, rows)
            self._gemm(pl.gemm[b + 'qkv'], d['f', b + 'qkv'], pl.ln)
            L.check(lib.rick_clip_attention_f32(self.qkv[i].data_ptr(), pl.att.data_ptr(), n, c.tokens, c.heads, c.width // c.heads,
                                                stream), 'rick_clip_attention_f32')
            self._gemm(pl.gemm[b + 'out'], d['f', b + 'out'], pl.att, res=t0)
            layernorm(b + 'ln2', t1, c.width, pl.ln, rows)
            self._gemm(pl.gemm[b + 'fc'], d['f', b + 'fc'], pl.ln)                # the pre-activation, kept
            L.check(lib.rick_clip_quickgelu_f32(self.pre[i].data_ptr(), pl.hid.data_ptr(), rows * c.mlp, stream), 'rick_clip_quickgelu_f32')
            self._gemm(pl.gemm[b + 'proj'], d['f', b + 'proj'], pl.hid, res=t1)
        layernorm('ln_post', self.res[-1], c.tokens * c.width, pl.post, n)
        run_fc(pl.post.data_ptr(), pl.head.data_ptr(), pl.head_bias.data_ptr(), pl.ws.data_ptr(), out.data_ptr(), n, c.width, c.dim, 0)

    def backward(self, go, gx):
        """go [n, D] -> gx [n, 3, H, W], the gradient with respect to the images of the last forward run."""
        L, c = self._lib, self.cfg
        lib, stream = L.lib, L.stream_ptr()
        n, _, H, W = gx.shape
        rows, d, v = n * c.tokens, self._descriptors(n), self.plan.vec
        wd = c.width

        def layernorm_bwd(name, x, ldx, g, add, ld, r):
            L.check(lib.rick_clip_layernorm_bwd_f32(x.data_ptr(), ldx, v[name + '.w'].data_ptr(), g.data_ptr(), wd,
                                                    None if add is None else add.data_ptr(), self.gt.data_ptr(), ld, r, wd, EPS, stream),
                    'rick_clip_layernorm_bwd_f32')

        run_fc(go.data_ptr(), self.head_t.data_ptr(), self.head_t_bias.data_ptr(), self.ws.data_ptr(), self.gpost.data_ptr(), n, c.dim, wd,
               0)
        self.gt[:rows * wd].zero_()                           # ln_post saw token 0 only
        layernorm_bwd('ln_post', self.res[-1], c.tokens * wd, self.gpost, None, c.tokens * wd, n)
        for i in reversed(range(c.layers)):
            b = f'blocks.{i}.'
            self._gemm(self.gemm[b + 'proj'], d['b', b + 'proj'], self.gt)
            L.check(lib.rick_clip_quickgelu_bwd_f32(self.pre[i].data_ptr(), self.gh.data_ptr(), self.gh.data_ptr(), rows * c.mlp, stream),
                    'rick_clip_quickgelu_bwd_f32')
            self._gemm(self.gemm[b + 'fc'], d['b', b + 'fc'], self.gh)
            layernorm_bwd(b + 'ln2', self.res[2 * i + 1], wd, self.ga, self.gt, wd, rows)
            self._gemm(self.gemm[b + 'out'], d['b', b + 'out'], self.gt)
            L.check(lib.rick_clip_attention_bwd_f32(self.qkv[i].data_ptr(), self.ga.data_ptr(), self.stats.data_ptr(), self.gq.data_ptr(),
                                                    n, c.tokens, c.heads, wd // c.heads, stream), 'rick_clip_attention_bwd_f32')
            self._gemm(self.gemm[b + 'qkv'], d['b', b + 'qkv'], self.gq)
            layernorm_bwd(b + 'ln1', self.res[2 * i], wd, self.ga, self.gt, wd, rows)
        L.check(lib.rick_clip_tokens_bwd_f32(self.patches.data_ptr(), v['pos'].data_ptr(), v['ln_pre.w'].data_ptr(), self.gt.data_ptr(),
                                             self.gp.data_ptr(), n, c.tokens, wd, EPS, stream), 'rick_clip_tokens_bwd_f32')
        self._gemm(self.gemm['patch'], d['b', 'patch'], self.gp)
        L.check(lib.rick_clip_input_bwd_f32(self.gx0.data_ptr(), gx.data_ptr(), n, H, W, c.size, c.patch, stream), 'rick_clip_input_bwd_f32')


class _Encode(torch.autograd.Function):
    """[N, D] embeddings of x; the gradient with respect to x on the HIP backward kernels."""

    @staticmethod
    def forward(ctx, x, net):
        ws = net._grad_workspace()
        x = x.contiguous()
        out = torch.empty((x.shape[0], net.cfg.dim), device=x.device, dtype=torch.float32)
        with torch.cuda.device(net.device):
            ws.forward(x, out)
        ctx.net, ctx.ws, ctx.version, ctx.shape = net, ws, ws.version, tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, go):
        if torch.is_grad_enabled():
            raise RuntimeError(f'{WHO}.encode: the backward pass is first order only (create_graph=True is not supported)')
        ws = ctx.net._grad_workspace()
        if ws is not ctx.ws or ws.version != ctx.version:
            raise RuntimeError(f'{WHO}.encode: the stored activations were overwritten by a later differentiable call; '
                               f'run backward before the next {WHO}.encode on this network')
        if go.device != ctx.net.device or go.dtype != torch.float32:
            raise RuntimeError(f'{WHO}.encode: upstream gradient on {go.device} / {go.dtype}')
        go = go.contiguous()
        gx = torch.empty(ctx.shape, device=go.device, dtype=torch.float32)
        with torch.cuda.device(ctx.net.device):
            ws.backward(go, gx)
        return gx, None


class ClipImageFeatures:
    """CLIP's ViT image tower up to the projection (unnormalised embeddings) on HIP kernels; see the module docstring."""

    def __init__(self, params, device='cuda', batch=25, heads=None):
        if batch < 1:
            raise ValueError(f'{WHO}: batch must be >= 1')
        self.params, self.cfg = params, config_from_params(params, heads)
        self.batch = int(batch)
        self.device = cuda_device(device)
        self._plan, self._grad_ws = None, None
        if self.device.type == 'cuda':
            with torch.cuda.device(self.device):
                self._plan = _Plan(params, self.cfg, self.batch, self.device)

    @classmethod
    def load(cls, src, device='cuda', batch=25, heads=None):
        """src: a path or state_dict in the transformers or the OpenAI layout."""
        return cls(params_from_state_dict(load_dict(src)), device=device, batch=batch, heads=heads)

    @torch.no_grad()
    def __call__(self, x):
        """x [N, 3, H, W] fp32 in [-1, 1] -> image embeddings [N, D] fp32 on x's device."""
        check_images(x, WHO, self.device)
        N = x.shape[0]
        if x.device.type == 'cpu':
            out = torch.empty((N, self.cfg.dim), dtype=torch.float32)
            for lo in range(0, N, self.batch):
                out[lo:lo + self.batch] = torch_forward(self.params, self.cfg, x[lo:lo + self.batch])
            return out
        out = torch.empty((N, self.cfg.dim), device=x.device, dtype=torch.float32)
        x = x.contiguous()
        with torch.cuda.device(self.device):
            for lo in range(0, N, self.batch):
                hi = min(N, lo + self.batch)
                self._plan.run(x[lo:hi], out[lo:hi])
        return out

    def prepare_grad(self, grad_batch=8):
        """Builds what ``encode`` needs for up to `grad_batch` images per differentiable call (at most `batch`): the transposed
        GEMM operands, packed once (about as much device memory again as the forward operands, 0.35 GB at ViT-B/32), one set of
        stored activations (about 17 MB per image at ViT-B/32) and the gradient buffers.  ``encode`` calls it with the default
        on first use.  ``__call__`` is not affected: same plan, same launches."""
        if self._plan is None:
            raise RuntimeError(f'{WHO}: prepare_grad needs a network loaded for a GPU (CPU tensors use torch autograd)')
        if self._grad_ws is None or self._grad_ws.batch != int(grad_batch):
            with torch.cuda.device(self.device):
                self._grad_ws = _GradWorkspace(self._plan, self.params, int(grad_batch), self.device)
        return self

    def _grad_workspace(self):
        if self._grad_ws is None:
            self.prepare_grad(min(8, self.batch))
        return self._grad_ws

    def encode(self, x):
        """``__call__``'s values, bit for bit, differentiable with respect to x when x requires grad (otherwise it IS
        ``__call__``).  First order only: ``create_graph=True`` raises in the backward pass.  CUDA tensors run the HIP backward
        kernels over one set of stored activations (``prepare_grad``): a differentiable call of more than grad_batch images
        raises (it is not chunked), and a backward pass must run before the next differentiable call on this network.  The
        weights are frozen: the only gradient is the image's.  CPU tensors take torch autograd through ``torch_forward``."""
        check_images(x, WHO, self.device)
        if not (x.requires_grad and torch.is_grad_enabled()):
            return self(x)
        if x.device.type == 'cpu':
            return torch_forward(self.params, self.cfg, x)
        ws = self._grad_workspace()
        if x.shape[0] > ws.batch:
            raise ValueError(f'{WHO}.encode: {x.shape[0]} images in a differentiable call, grad_batch is {ws.batch} '
                             f'(prepare_grad(grad_batch=...); the call is not chunked)')
        return _Encode.apply(x, self)
