"""CLIP's text tower (Radford et al., 2021) on HIP kernels: the unnormalised text embeddings that ``encode_text`` returns,
for text-derived directions of the CLIP-guided adaptation losses (rick_amd/clipguide.py ``text_direction``).  Forward only:
the weights are frozen and the input is discrete, so there is nothing to differentiate.

    tnet = ClipTextFeatures.load(src, device='cuda', batch=64)       # src: a state_dict or a path, either layout below
    ids = ClipTokenizer.load(vocab_json, merges_txt)(['a photo of a dog'])                   # rick_amd/cliptok.py
    e = tnet(ids)                               # ids [N, T] integer (CPU or CUDA) -> [N, D] fp32, unnormalised

The network, per prompt:

1. tokens = token_embedding[ids] + positional_embedding [T, Wd]; no class token, no ln_pre;
2. L blocks, the image tower's (rick_amd/clip.py) with causal attention: t += out_proj(attn(ln_1(t)));
   t += c_proj(quickgelu(c_fc(ln_2(t)))); query row i sees the keys k <= i;
3. ``ln_final`` (eps 1e-5) on the row at argmax(ids), the first occurrence of the maximum: CLIP's rule, EOT being the largest
   id of the vocabulary.  `transformers` takes the first ``eos_token_id``: the same row whenever EOT is the row's largest id;
4. ``text_projection`` without bias -> [N, D].

Rows behind the EOT row cannot reach it under the causal mask, so the padding value does not matter.

CUDA ids run rick_clip_text_tokens_f32, per layer rick_clip_layernorm_f32 (twice), rick_inc_conv_lin_f32 (the fused q/k/v
projection, out_proj and c_proj with the residual, c_fc with QuickGELU) and rick_clip_attention_causal_f32, then
rick_clip_layernorm_rows_f32 on the EOT rows and rick_fc_f32 (include/rick_hip.h "CLIP").  The ids are validated on the host,
which also finds the EOT rows; both go to the device in one copy.  A prompt's embedding is bit-identical whatever batch it is
computed in, and from run to run.  The workspace for ``batch`` prompts and every packed operand are allocated once at
construction; larger inputs are chunked.  CPU ids run the same network as a plain fp32 torch composition
(``torch_text_forward``).  The blocks, their loader and their launches are the image tower's too (rick_amd/cliptower.py).

``src`` is a state_dict in one of two layouts, cast to fp32:

* transformers (``CLIPModel`` / ``CLIPTextModelWithProjection``): ``text_model.embeddings.{token_embedding,
  position_embedding}.weight``, ``text_model.encoder.layers.{i}.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.fc1,
  mlp.fc2}.*``, ``text_model.final_layer_norm.*``, ``text_projection.weight [D, Wd]``;
* OpenAI: ``token_embedding.weight``, ``positional_embedding``, ``transformer.resblocks.{i}.{ln_1.*, attn.in_proj_{weight
  [3 Wd, Wd] (rows q, k, v), bias}, attn.out_proj.*, ln_2.*, mlp.c_fc.*, mlp.c_proj.*}``, ``ln_final.*``,
  ``text_projection [Wd, D]``.

Image-tower keys (``vision_model.*``, ``visual_projection.weight``, ``visual.*``), ``logit_scale``, ``position_ids`` and
OpenAI's scalar entries are ignored, so a whole-model checkpoint loads into both towers; any other unknown key raises.  The
configuration is read from the shapes; heads = Wd / 64 (CLIP's rule) unless ``heads`` is given.  Supported: head dim in
{16, 32, 64}, T <= 257, Wd and the MLP width multiples of 4, Wd <= 2048.
"""
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from .cliptower import (CAUSAL_ATTENTION, EPS, Transformer, blocks_from_state_dict, head_from_state_dict, issue, launch, limits,
                        refuse_unexpected, shape, torch_blocks)
from .netutil import cuda_device, get, load_dict

WHO = 'ClipTextFeatures'

TextConfig = namedtuple('TextConfig', 'width tokens vocab layers mlp dim heads')

# ---- loading --------------------------------------------------------------------------------------------------------------
_get = functools.partial(get, who=WHO, errors=(RuntimeError, RuntimeError))
_IGNORED_PREFIX = ('vision_model.', 'visual.')
_IGNORED = ('visual_projection.weight', 'logit_scale', 'input_resolution', 'context_length', 'vocab_size')


def params_from_state_dict(sd):
    """Either layout -> the network's parameters as fp32 CPU tensors under layout-free names: tok [V, Wd], pos [T, Wd],
    blocks.{i}.{ln1.{w,b}, qkv.{w [3 Wd, Wd], b}, out.{w,b}, ln2.{w,b}, fc.{w [M, Wd], b}, proj.{w [Wd, M], b}}, ln_final.{w,b},
    head [D, Wd]."""
    hf = any(k.startswith('text_model.') for k in sd)
    if hf:
        k_tok, k_pos = 'text_model.embeddings.token_embedding.weight', 'text_model.embeddings.position_embedding.weight'
        pre, k_ln, k_head = 'text_model.encoder.layers.', 'text_model.final_layer_norm', 'text_projection.weight'
    else:
        k_tok, k_pos = 'token_embedding.weight', 'positional_embedding'
        pre, k_ln, k_head = 'transformer.resblocks.', 'ln_final', 'text_projection'
    tshape = shape(sd, k_tok, WHO)
    if len(tshape) != 2:
        raise RuntimeError(f'{WHO}: key {k_tok!r} has shape {tshape}, expected (V, Wd)')
    wd = tshape[1]
    pshape = shape(sd, k_pos, WHO)
    if len(pshape) != 2 or pshape[1] != wd:
        raise RuntimeError(f'{WHO}: key {k_pos!r} has shape {pshape}, expected (T, {wd})')
    p = {'tok': _get(sd, k_tok, tshape), 'pos': _get(sd, k_pos, pshape)}
    for s, suffix in (('w', 'weight'), ('b', 'bias')):
        p[f'ln_final.{s}'] = _get(sd, f'{k_ln}.{suffix}', (wd,))
    blocks, keys = blocks_from_state_dict(sd, pre, hf, wd, WHO)
    p.update(blocks)
    p['head'] = head_from_state_dict(sd, k_head, hf, wd, WHO)
    refuse_unexpected(sd, keys | {k_tok, k_pos, k_ln + '.weight', k_ln + '.bias', k_head},
                      lambda k: k.startswith(_IGNORED_PREFIX) or k in _IGNORED or k.endswith('position_ids'), WHO)
    return p


def config_from_params(p, heads=None):
    """The configuration the shapes imply; refuses what the kernels do not support."""
    vocab, wd = p['tok'].shape
    tokens = p['pos'].shape[0]
    if tokens < 1:
        raise RuntimeError(f'{WHO}: positional embedding has {tokens} rows, expected at least 1')
    layers, mlp, heads = limits(p, wd, tokens, heads, 'positions per prompt', WHO)
    return TextConfig(wd, tokens, vocab, layers, mlp, p['head'].shape[0], heads)


# ---- the ids ----------------------------------------------------------------------------------------------------------------
def check_ids(ids, cfg, device=None):
    """ids must be [N, T] of an integer dtype with T the positional embedding's rows and every id in [0, V), on the CPU or on
    `device` -> the ids as int64 on the CPU."""
    if ids.dim() != 2:
        raise RuntimeError(f'{WHO}: expected ids [N, {cfg.tokens}], got {tuple(ids.shape)}')
    if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
        raise RuntimeError(f'{WHO}: ids must be of an integer dtype, got {ids.dtype}')
    if ids.shape[1] != cfg.tokens:
        raise ValueError(f'{WHO}: ids have {ids.shape[1]} positions, the positional embedding has {cfg.tokens}')
    if device is not None and ids.device.type != 'cpu' and ids.device != device:
        raise RuntimeError(f'{WHO}: ids on {ids.device}, network loaded for {device}')
    host = ids.detach().to('cpu', torch.int64)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= cfg.vocab):
        bad = host[(host < 0) | (host >= cfg.vocab)][0]
        raise ValueError(f'{WHO}: id {int(bad)} is outside the vocabulary [0, {cfg.vocab})')
    return host


def eot_positions(ids):
    """ids [N, T] int64 -> [N] int64, the first position of each row's maximum (CLIP's EOT rule)."""
    first = (ids == ids.max(1, keepdim=True).values).to(torch.int64)
    return (first.cumsum(1) == 0).sum(1)                      # the positions in front of the first maximum


def check_rows(idx, rows):
    """idx: integer row numbers for rick_clip_layernorm_rows_f32 over `rows` rows -> int32 CPU; refuses what is out of range."""
    idx = torch.as_tensor(idx)
    if idx.dim() != 1 or idx.dtype.is_floating_point or idx.dtype == torch.bool:
        raise RuntimeError(f'{WHO}: expected integer row numbers [R], got {tuple(idx.shape)} {idx.dtype}')
    host = idx.detach().to('cpu', torch.int64)
    if host.numel() and (int(host.min()) < 0 or int(host.max()) >= rows):
        bad = host[(host < 0) | (host >= rows)][0]
        raise ValueError(f'{WHO}: row {int(bad)} is outside the {rows} rows of the input')
    return host.to(torch.int32)


def layernorm_rows(x, idx, w, b, eps=EPS):
    """LayerNorm of the rows idx [R] (integer, checked on the host before upload) of x [rows, C] CUDA fp32 contiguous ->
    [R, C]: rick_clip_layernorm_rows_f32, the bits of rick_clip_layernorm_f32 on the gathered rows."""
    from . import _lib as L
    L.require_cuda_f32(x, w, b)
    if x.dim() != 2 or not x.is_contiguous() or w.shape != (x.shape[1],) or b.shape != (x.shape[1],):
        raise RuntimeError(f'{WHO}: expected contiguous rows [R, C] and w, b [C], got {tuple(x.shape)}, {tuple(w.shape)}, {tuple(b.shape)}')
    host = check_rows(idx, x.shape[0])
    with torch.cuda.device(x.device):
        dev = host.to(x.device)
        out = torch.empty((host.numel(), x.shape[1]), device=x.device, dtype=torch.float32)
        L.check(L.lib.rick_clip_layernorm_rows_f32(x.data_ptr(), dev.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), host.numel(),
                                                   x.shape[1], eps, L.stream_ptr()), 'rick_clip_layernorm_rows_f32')
    return out


# ---- the network as a plain torch composition -----------------------------------------------------------------------------
def torch_text_forward(p, cfg, ids):
    """The whole network on ids [N, T] int64, in the dtype and on the device of the parameters p -> [N, D]."""
    t = p['tok'][ids] + p['pos']
    mask = torch.full((cfg.tokens, cfg.tokens), -math.inf, dtype=t.dtype, device=t.device).triu(1)
    t = torch_blocks(p, cfg, t, mask)
    rows = t[torch.arange(ids.shape[0], device=t.device), eot_positions(ids)]
    return F.linear(F.layer_norm(rows, (cfg.width,), p['ln_final.w'], p['ln_final.b'], EPS), p['head'])


# ---- device plan ----------------------------------------------------------------------------------------------------------
class _Plan:
    """Packed operands and the workspace of `batch` prompts on the device.

    Per prompt: T + 1 int32 (the ids and the EOT row), and per token, in floats, the residual stream Wd, the LayerNorm output
    Wd, q|k|v 3 Wd, the attention output Wd and the MLP's hidden layer: 1.6 MB per prompt at ViT-B/32's text tower (T = 77,
    Wd = 512, MLP 2048), 0.1 GB at the default 64, next to 0.15 GB of packed weights and the 0.1 GB embedding table."""

    def __init__(self, p, cfg, batch, device):
        self.cfg, self.batch, self.fwd = cfg, batch, {}
        self.tf = Transformer(p, cfg, batch, device, WHO, CAUSAL_ATTENTION, tables=('pos', 'tok'))     # in place, as the image tower
        self.ids = torch.empty(batch * cfg.tokens + batch, device=device, dtype=torch.int32)      # [batch, T] ids, then [batch] EOT rows

    def upload(self, ids):
        """ids [n, T] int64 CPU, validated -> the device's id block: the ids, then row n' T + eot(n') of every prompt."""
        n, T = ids.shape
        eot = check_rows(torch.arange(n) * T + eot_positions(ids), n * T)
        self.ids[:n * T + n].copy_(torch.cat([ids.reshape(-1).to(torch.int32), eot]))

    def run(self, n, out):
        """The n prompts of the last upload -> out [n, D] (contiguous rows); the launches are resolved once per n."""
        if n not in self.fwd:
            c, tf, v = self.cfg, self.tf, self.tf.vec
            self.fwd[n] = [launch('tokens', 'rick_clip_text_tokens_f32', self.ids.data_ptr(), v['tok'].data_ptr(), v['pos'].data_ptr(),
                                  tf.tok.data_ptr(), n, c.tokens, c.vocab, c.width),
                           *tf.launches(n),
                           launch('ln_final', 'rick_clip_layernorm_rows_f32', tf.tok.data_ptr(), self.ids.data_ptr() + 4 * n * c.tokens,
                                  v['ln_final.w'].data_ptr(), v['ln_final.b'].data_ptr(), tf.post.data_ptr(), n, c.width, EPS)]
        issue(self.fwd[n])
        self.tf.project(n, out)


class ClipTextFeatures:
    """CLIP's text tower up to the projection (unnormalised embeddings) on HIP kernels; see the module docstring."""

    def __init__(self, params, device='cuda', batch=64, heads=None):
        if batch < 1:
            raise ValueError(f'{WHO}: batch must be >= 1')
        self.params, self.cfg = params, config_from_params(params, heads)
        self.batch = int(batch)
        self.device = cuda_device(device)
        self._plan = None
        if self.device.type == 'cuda':
            with torch.cuda.device(self.device):
                self._plan = _Plan(params, self.cfg, self.batch, self.device)

    @classmethod
    def load(cls, src, device='cuda', batch=64, heads=None):
        """src: a path or state_dict in the transformers or the OpenAI layout."""
        return cls(params_from_state_dict(load_dict(src)), device=device, batch=batch, heads=heads)

    @torch.no_grad()
    def __call__(self, ids):
        """ids [N, T] of an integer dtype, every id in [0, V) -> text embeddings [N, D] fp32 on the ids' device."""
        host = check_ids(ids, self.cfg, self.device)
        N = host.shape[0]
        if ids.device.type == 'cpu':
            out = torch.empty((N, self.cfg.dim), dtype=torch.float32)
            for lo in range(0, N, self.batch):
                out[lo:lo + self.batch] = torch_text_forward(self.params, self.cfg, host[lo:lo + self.batch])
            return out
        out = torch.empty((N, self.cfg.dim), device=ids.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            for lo in range(0, N, self.batch):
                hi = min(N, lo + self.batch)
                self._plan.upload(host[lo:hi])
                self._plan.run(hi - lo, out[lo:hi])
        return out
