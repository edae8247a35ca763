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
CPU tensors run the same network as a plain fp32 torch composition (``torch_forward``).  The blocks, their loader and their
launches are the text tower's too (rick_amd/cliptower.py).

``src`` is a state_dict in one of two layouts, cast to fp32 (OpenAI checkpoints are fp16):

* transformers (``CLIPModel`` / ``CLIPVisionModelWithProjection``): ``vision_model.embeddings.{class_embedding,
  patch_embedding.weight, position_embedding.weight}``, ``vision_model.pre_layrnorm.*`` (the library's spelling),
  ``vision_model.encoder.layers.{i}.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.fc1, mlp.fc2}.*``,
  ``vision_model.post_layernorm.*``, ``visual_projection.weight [D, Wd]``;
* OpenAI, with or without the ``visual.`` prefix: ``conv1.weight``, ``class_embedding``, ``positional_embedding``,
  ``ln_pre.*``, ``transformer.resblocks.{i}.{ln_1.*, attn.in_proj_{weight [3 Wd, Wd] (rows q, k, v), bias},
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
from .cliptower import (ATTENTION, EPS, HEAD_DIMS, MAX_TOKENS, MAX_WIDTH, Transformer, blocks_from_state_dict,     # noqa: F401
                        column_block, fc_workspace, gemm, head_from_state_dict, issue, launch, limits, linear, operand, pack_linear,
                        refuse_unexpected, shape, torch_blocks)
from .fc import check_packed, pack_fc_weight, run_fc
from .netutil import check_images, cuda_device, get, load_dict

WHO = 'ClipImageFeatures'
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)

ClipConfig = namedtuple('ClipConfig', 'width patch tokens grid size layers mlp dim heads')

# ---- loading --------------------------------------------------------------------------------------------------------------
_get = functools.partial(get, who=WHO, errors=(RuntimeError, RuntimeError))
_OPENAI_TEXT = ('token_embedding.', 'ln_final.', 'text_projection', 'logit_scale', 'input_resolution', 'context_length', 'vocab_size')


def params_from_state_dict(sd):
    """Either layout -> the network's parameters as fp32 CPU tensors under layout-free names: conv1 [Wd, 3, P, P], cls [Wd],
    pos [T, Wd], ln_pre.{w,b}, blocks.{i}.{ln1.{w,b}, qkv.{w [3 Wd, Wd], b}, out.{w,b}, ln2.{w,b}, fc.{w [M, Wd], b},
    proj.{w [Wd, M], b}}, ln_post.{w,b}, head [D, Wd]."""
    hf = any(k.startswith('vision_model.') for k in sd)
    used, p = set(), {}

    def take(name, key, shape_):
        p[name] = _get(sd, key, shape_)
        used.add(key)

    if hf:
        emb, pre = 'vision_model.embeddings.', 'vision_model.encoder.layers.'
        k_conv, k_cls, k_pos = emb + 'patch_embedding.weight', emb + 'class_embedding', emb + 'position_embedding.weight'
        k_lnpre, k_lnpost, k_head = 'vision_model.pre_layrnorm', 'vision_model.post_layernorm', 'visual_projection.weight'
        ignored = lambda k: (k.startswith('text_model.') or k in ('text_projection.weight', 'logit_scale')      # noqa: E731
                             or k.endswith('position_ids'))
    else:
        v = 'visual.' if 'visual.conv1.weight' in sd else ''
        pre = v + 'transformer.resblocks.'
        k_conv, k_cls, k_pos = v + 'conv1.weight', v + 'class_embedding', v + 'positional_embedding'
        k_lnpre, k_lnpost, k_head = v + 'ln_pre', v + 'ln_post', v + 'proj'
        # beside a prefixed image tower, the unprefixed transformer and positional embedding are the text tower's
        ignored = lambda k: (k.startswith(_OPENAI_TEXT) or k.endswith('position_ids')                           # noqa: E731
                             or (v and (k.startswith('transformer.') or k == 'positional_embedding')))
    cshape = shape(sd, k_conv, WHO)
    if len(cshape) != 4 or cshape[1] != 3 or cshape[2] != cshape[3]:
        raise RuntimeError(f'{WHO}: key {k_conv!r} has shape {cshape}, expected (Wd, 3, P, P)')
    wd = cshape[0]
    pshape = shape(sd, k_pos, WHO)
    take('conv1', k_conv, cshape)
    take('cls', k_cls, (wd,))
    take('pos', k_pos, (pshape[0], wd) if len(pshape) == 2 else (0, wd))
    for name, key in (('ln_pre', k_lnpre), ('ln_post', k_lnpost)):
        for s, suffix in (('w', 'weight'), ('b', 'bias')):
            take(f'{name}.{s}', f'{key}.{suffix}', (wd,))
    blocks, keys = blocks_from_state_dict(sd, pre, hf, wd, WHO)
    p.update(blocks)
    p['head'] = head_from_state_dict(sd, k_head, hf, wd, WHO)
    refuse_unexpected(sd, used | keys | {k_head}, ignored, WHO)
    return p


def config_from_params(p, heads=None):
    """The configuration the shapes imply; refuses what the kernels do not support."""
    wd, _, patch, _ = p['conv1'].shape
    tokens = p['pos'].shape[0]
    grid = math.isqrt(max(tokens - 1, 0))
    if tokens <= MAX_TOKENS and (tokens < 2 or grid * grid + 1 != tokens):
        raise RuntimeError(f'{WHO}: positional embedding has {tokens} rows, expected G^2 + 1')
    layers, mlp, heads = limits(p, wd, tokens, heads, 'tokens per image', WHO)
    return ClipConfig(wd, patch, tokens, grid, grid * patch, layers, mlp, p['head'].shape[0], heads)


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
    wd = cfg.width
    t = torch.cat([p['cls'].expand(t.shape[0], 1, wd), t], 1) + p['pos']
    t = torch_blocks(p, cfg, F.layer_norm(t, (wd,), p['ln_pre.w'], p['ln_pre.b'], EPS))
    return F.linear(F.layer_norm(t[:, 0], (wd,), p['ln_post.w'], p['ln_post.b'], EPS), p['head'])


# ---- GEMM operands --------------------------------------------------------------------------------------------------------
def pack_patch_embedding(w, bn=None):
    """conv1 [Wd, 3, P, P] -> the operand of the P x P stride-P convolution on the NHWC4 input: rows (ky, kx, c) with c < 4 and
    a zero row for c = 3.  No bias.  (wpk, bias, Cop, bn)."""
    return gemm_conv.pack(w, None, ci_pad=4, bn=bn)


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


# ---- device plan ----------------------------------------------------------------------------------------------------------
def _forward(s, x, out):
    """x [n, 3, H, W] fp32 contiguous, n <= batch -> out [n, D] (contiguous rows) on the buffers of s, a _Plan or a
    _GradWorkspace: its input x0, its patch rows and the residual streams, q|k|v and pre-activations of its Transformer s.tf.
    Everything but the input kernel, which reads x, is resolved once per n."""
    from . import _lib as L
    c, tf = s.cfg, s.tf
    n, _, H, W = x.shape
    if n not in s.fwd:
        v, P = tf.vec, (c.patch, c.patch)
        _, _, cop, bn = s.patch
        a = gemm_conv.descriptor(n, c.size, c.size, 4, P, P, (0, 0), cop, bn, [(s.patches.data_ptr(), c.width, 0, c.width)])
        s.fwd[n] = [gemm('patch', s.patch, a, s.x0),
                    launch('tokens', 'rick_clip_tokens_f32', s.patches.data_ptr(), v['cls'].data_ptr(), v['pos'].data_ptr(),
                           v['ln_pre.w'].data_ptr(), v['ln_pre.b'].data_ptr(), tf.res[0].data_ptr(), n, c.tokens, c.width, EPS),
                    *tf.launches(n),
                    tf.layernorm('ln_post', 'ln_post', tf.res[-1], c.tokens * c.width, tf.post, n)]     # token 0 of every image
    stream = L.stream_ptr()
    L.check(L.lib.rick_clip_input_f32(x.data_ptr(), s.x0.data_ptr(), n, H, W, c.size, stream), 'rick_clip_input_f32')
    issue(s.fwd[n], stream)
    tf.project(n, out)


class _Plan:
    """Packed operands and the workspace of `batch` images on the device.

    Per image, in floats: the NHWC4 input 4 S^2, the patch rows G^2 Wd, and per token the residual stream Wd, the LayerNorm
    output Wd, q|k|v 3 Wd, the attention output Wd and the MLP's hidden layer: 2.5 MB per image at ViT-B/32, 62 MB at the default
    25, next to 0.35 GB of packed weights."""

    def __init__(self, p, cfg, batch, device):
        self.cfg, self.batch, self.fwd = cfg, batch, {}
        self.patch = operand(pack_patch_embedding(p['conv1'], column_block(cfg.width, batch * (cfg.tokens - 1))), device)
        self.tf = Transformer(p, cfg, batch, device, WHO, ATTENTION,      # in place: the one residual stream, the one q|k|v
                              stem=(batch * cfg.size * cfg.size * 4, batch * (cfg.tokens - 1) * cfg.width))
        self.x0, self.patches = self.tf.stem

    def run(self, x, out):
        _forward(self, x, out)


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
        self.cfg, self.batch, self.version, self.patch, self.fwd, self.bwd = plan.cfg, int(batch), 0, plan.patch, {}, {}
        c, f32 = self.cfg, dict(device=device, dtype=torch.float32)
        rows = batch * c.tokens
        self.patch_t = operand(pack_patch_embedding_transposed(p['conv1'], column_block(4 * c.patch * c.patch, batch * (c.tokens - 1))),
                               device)

        def transposed(w):
            return operand(pack_linear_transposed(w, column_block(w.shape[1], rows)), device)

        self.gemm = [{name: transposed(p[f'blocks.{i}.{name}.w']) for name in ('qkv', 'out', 'fc', 'proj')} for i in range(c.layers)]
        head_t = pack_fc_weight(p['head'].t().contiguous())
        check_packed(head_t, c.dim, c.width, WHO)
        self.head_t, self.head_t_bias = head_t.to(device), torch.zeros(c.width, **f32)
        buf = lambda n: torch.empty(n, **f32)                                     # noqa: E731
        self.x0, self.patches = buf(batch * c.size * c.size * 4), buf(batch * (c.tokens - 1) * c.width)
        self.res = [buf(rows * c.width) for _ in range(2 * c.layers + 1)]
        self.qkv = [buf(rows * 3 * c.width) for _ in range(c.layers)]
        self.pre = [buf(rows * c.mlp) for _ in range(c.layers)]
        self.tf = plan.tf.wired(self.res, self.qkv, self.pre)
        self.gt, self.ga, self.gh, self.gq = buf(rows * c.width), buf(rows * c.width), buf(rows * c.mlp), buf(rows * 3 * c.width)
        self.stats = buf(batch * c.heads * c.tokens * 3)
        self.gpost, self.gp, self.gx0 = buf(batch * c.width), buf(batch * (c.tokens - 1) * c.width), buf(batch * c.size * c.size * 4)
        self.ws = buf(fc_workspace(batch, c.dim, c.width))

    def forward(self, x, out):
        """_Plan.run with the activations kept: x [n, 3, H, W] fp32 contiguous, n <= batch -> out [n, D], the same bits."""
        self.version += 1
        _forward(self, x, out)

    def backward_launches(self, n):
        """The backward pass of n images between the projection's adjoint and the input's, resolved once per n."""
        if n not in self.bwd:
            c, v = self.cfg, self.tf.vec
            rows, wd, k2 = n * c.tokens, c.width, 4 * c.patch * c.patch

            def ln_bwd(name, x, ldx, g, add, ld, r):
                return launch('ln_bwd', 'rick_clip_layernorm_bwd_f32', x.data_ptr(), ldx, v[name + '.w'].data_ptr(), g.data_ptr(), wd,
                              None if add is None else add.data_ptr(), self.gt.data_ptr(), ld, r, wd, EPS)

            out = [ln_bwd('ln_post', self.res[-1], c.tokens * wd, self.gpost, None, c.tokens * wd, n)]
            for i in reversed(range(c.layers)):
                b, op = f'blocks.{i}.', self.gemm[i]
                out += [linear('proj^T', op['proj'], rows, wd, c.mlp, self.gt, self.gh),
                        launch('quickgelu_bwd', 'rick_clip_quickgelu_bwd_f32', self.pre[i].data_ptr(), self.gh.data_ptr(),
                               self.gh.data_ptr(), rows * c.mlp),
                        linear('fc^T', op['fc'], rows, c.mlp, wd, self.gh, self.ga),
                        ln_bwd(b + 'ln2', self.res[2 * i + 1], wd, self.ga, self.gt, wd, rows),
                        linear('out^T', op['out'], rows, wd, wd, self.gt, self.ga),
                        launch('attention_bwd', 'rick_clip_attention_bwd_f32', self.qkv[i].data_ptr(), self.ga.data_ptr(),
                               self.stats.data_ptr(), self.gq.data_ptr(), n, c.tokens, c.heads, wd // c.heads),
                        linear('qkv^T', op['qkv'], rows, 3 * wd, wd, self.gq, self.ga),
                        ln_bwd(b + 'ln1', self.res[2 * i], wd, self.ga, self.gt, wd, rows)]
            out += [launch('tokens_bwd', 'rick_clip_tokens_bwd_f32', self.patches.data_ptr(), v['pos'].data_ptr(), v['ln_pre.w'].data_ptr(),
                           self.gt.data_ptr(), self.gp.data_ptr(), n, c.tokens, wd, EPS),
                    linear('patch^T', self.patch_t, n * (c.tokens - 1), wd, k2, self.gp, self.gx0)]
            self.bwd[n] = out
        return self.bwd[n]

    def backward(self, go, gx):
        """go [n, D] -> gx [n, 3, H, W], the gradient with respect to the images of the last forward run."""
        from . import _lib as L
        c = self.cfg
        n, _, H, W = gx.shape
        run_fc(go.data_ptr(), self.head_t.data_ptr(), self.head_t_bias.data_ptr(), self.ws.data_ptr(), self.gpost.data_ptr(), n, c.dim,
               c.width, 0)
        self.gt[:n * c.tokens * c.width].zero_()              # ln_post saw token 0 only
        stream = L.stream_ptr()
        issue(self.backward_launches(n), stream)
        L.check(L.lib.rick_clip_input_bwd_f32(self.gx0.data_ptr(), gx.data_ptr(), n, H, W, c.size, c.patch, stream), 'rick_clip_input_bwd_f32')


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
