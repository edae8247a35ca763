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
(``torch_text_forward``).

``src`` is a state_dict in one of two layouts, cast to fp32:

* transformers (``CLIPModel`` / ``CLIPTextModelWithProjection``): ``text_model.embeddings.{token_embedding,
  position_embedding}.weight``, ``text_model.encoder.layers.{i}.{layer_norm1, self_attn.{q,k,v,out}_proj, layer_norm2, mlp.fc1,
  mlp.fc2}.*``, ``text_model.final_layer_norm.*``, ``text_projection.weight [D, Wd]``;
* OpenAI: ``token_embedding.weight``, ``positional_embedding``, ``transformer.resblocks.{i}.{ln_1.*, attn.in_proj_weight
  [3 Wd, Wd] (rows q, k, v), attn.in_proj_bias, attn.out_proj.*, ln_2.*, mlp.c_fc.*, mlp.c_proj.*}``, ``ln_final.*``,
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

from . import gemm_conv
from .clip import EPS, HEAD_DIMS, MAX_TOKENS, MAX_WIDTH, column_block, pack_linear
from .fc import FC_MAX_ROWS, check_packed, pack_fc_weight, run_fc
from .netutil import cuda_device, get, load_dict

WHO = 'ClipTextFeatures'

TextConfig = namedtuple('TextConfig', 'width tokens vocab layers mlp dim heads')

# ---- loading --------------------------------------------------------------------------------------------------------------
_get = functools.partial(get, who=WHO, errors=(RuntimeError, RuntimeError))
_IGNORED_PREFIX = ('vision_model.', 'visual.')
_IGNORED = ('visual_projection.weight', 'logit_scale', 'input_resolution', 'context_length', 'vocab_size')
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
    """Either layout -> the network's parameters as fp32 CPU tensors under layout-free names: tok [V, Wd], pos [T, Wd],
    blocks.{i}.{ln1.{w,b}, qkv.{w [3 Wd, Wd], b}, out.{w,b}, ln2.{w,b}, fc.{w [M, Wd], b}, proj.{w [Wd, M], b}}, ln_final.{w,b},
    head [D, Wd]."""
    hf = any(k.startswith('text_model.') for k in sd)
    used, p = set(), {}

    def take(name, key, shape):
        p[name] = _get(sd, key, shape)
        used.add(key)

    if hf:
        k_tok, k_pos = 'text_model.embeddings.token_embedding.weight', 'text_model.embeddings.position_embedding.weight'
        pre, k_ln, k_head, block = 'text_model.encoder.layers.', 'text_model.final_layer_norm', 'text_projection.weight', _BLOCK_HF
    else:
        k_tok, k_pos = 'token_embedding.weight', 'positional_embedding'
        pre, k_ln, k_head, block = 'transformer.resblocks.', 'ln_final', 'text_projection', _BLOCK_OPENAI
    tshape = _shape(sd, k_tok)
    if len(tshape) != 2:
        raise RuntimeError(f'{WHO}: key {k_tok!r} has shape {tshape}, expected (V, Wd)')
    wd = tshape[1]
    pshape = _shape(sd, k_pos)
    if len(pshape) != 2 or pshape[1] != wd:
        raise RuntimeError(f'{WHO}: key {k_pos!r} has shape {pshape}, expected (T, {wd})')
    take('tok', k_tok, tshape)
    take('pos', k_pos, pshape)
    for s, suffix in (('w', 'weight'), ('b', 'bias')):
        take(f'ln_final.{s}', f'{k_ln}.{suffix}', (wd,))
    layers = _layer_count(sd.keys(), pre)
    for i in range(layers):
        src, dst = f'{pre}{i}.', f'blocks.{i}.'
        mlp = _shape(sd, f'{src}{block["fc"]}.weight')[0]
        if hf:
            parts = []
            for suffix, shape in (('weight', (wd, wd)), ('bias', (wd,))):
                for proj in 'qkv':
                    key = f'{src}self_attn.{proj}_proj.{suffix}'
                    parts.append(_get(sd, key, shape))
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
        p['head'] = p['head'].t().contiguous()                # OpenAI's text_projection is [Wd, D]
    extra = sorted(k for k in sd if k not in used and not (k.startswith(_IGNORED_PREFIX) or k in _IGNORED or k.endswith('position_ids')))
    if extra:
        raise RuntimeError(f'{WHO}: unexpected key {extra[0]!r} in the state_dict')
    return p


def config_from_params(p, heads=None):
    """The configuration the shapes imply; refuses what the kernels do not support."""
    vocab, wd = p['tok'].shape
    tokens = p['pos'].shape[0]
    if tokens > MAX_TOKENS:
        raise RuntimeError(f'{WHO}: {tokens} positions per prompt, at most {MAX_TOKENS} are supported')
    if tokens < 1:
        raise RuntimeError(f'{WHO}: positional embedding has {tokens} rows, expected at least 1')
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
    return TextConfig(wd, tokens, vocab, layers, mlp, p['head'].shape[0], int(heads))


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
    wd, d, T = cfg.width, cfg.width // cfg.heads, cfg.tokens
    n = ids.shape[0]
    t = p['tok'][ids] + p['pos']
    mask = torch.full((T, T), -math.inf, dtype=t.dtype, device=t.device).triu(1)
    for i in range(cfg.layers):
        b = f'blocks.{i}.'
        h = F.layer_norm(t, (wd,), p[b + 'ln1.w'], p[b + 'ln1.b'], EPS)
        q, k, v = (u.view(n, T, cfg.heads, d).transpose(1, 2) for u in F.linear(h, p[b + 'qkv.w'], p[b + 'qkv.b']).split(wd, 2))
        a = torch.softmax(q @ k.transpose(2, 3) * (1.0 / math.sqrt(d)) + mask, -1) @ v
        t = t + F.linear(a.transpose(1, 2).reshape(n, T, wd), p[b + 'out.w'], p[b + 'out.b'])
        h = F.linear(F.layer_norm(t, (wd,), p[b + 'ln2.w'], p[b + 'ln2.b'], EPS), p[b + 'fc.w'], p[b + 'fc.b'])
        t = t + F.linear(h * torch.sigmoid(1.702 * h), p[b + 'proj.w'], p[b + 'proj.b'])
    rows = t[torch.arange(n, device=t.device), eot_positions(ids)]
    return F.linear(F.layer_norm(rows, (wd,), p['ln_final.w'], p['ln_final.b'], EPS), p['head'])


# ---- device plan ----------------------------------------------------------------------------------------------------------
class _Plan:
    """Packed operands and the workspace of `batch` prompts on the device.

    Per prompt: T + 1 int32 (the ids and the EOT row), and per token, in floats, the residual stream Wd, the LayerNorm output
    Wd, q|k|v 3 Wd, the attention output Wd and the MLP's hidden layer: 1.6 MB per prompt at ViT-B/32's text tower (T = 77,
    Wd = 512, MLP 2048), 0.1 GB at the default 64, next to 0.15 GB of packed weights and the 0.1 GB embedding table."""

    def __init__(self, p, cfg, batch, device):
        from . import _lib
        self._lib = _lib
        self.cfg, self.batch = cfg, batch
        f32 = dict(device=device, dtype=torch.float32)
        self.vec = {k: v.to(device) for k, v in p.items() if v.dim() == 1 or k in ('pos', 'tok')}
        self.gemm = {}
        rows = batch * cfg.tokens
        for i in range(cfg.layers):
            for name in ('qkv', 'out', 'fc', 'proj'):
                w = p[f'blocks.{i}.{name}.w']
                wpk, bias, cop, bn = pack_linear(w, p[f'blocks.{i}.{name}.b'], column_block(w.shape[0], rows))
                self.gemm[f'blocks.{i}.{name}'] = (wpk.to(device), bias.to(device), cop, bn)
        head = pack_fc_weight(p['head'])
        check_packed(head, cfg.width, cfg.dim, WHO)
        self.head, self.head_bias = head.to(device), torch.zeros(cfg.dim, **f32)
        self.ids = torch.empty(rows + batch, device=device, dtype=torch.int32)      # [batch, T] ids, then [batch] EOT rows
        self.tok, self.ln, self.att = (torch.empty(rows * cfg.width, **f32) for _ in range(3))
        self.qkv = torch.empty(rows * 3 * cfg.width, **f32)
        self.hid = torch.empty(rows * cfg.mlp, **f32)
        self.post = torch.empty(batch * cfg.width, **f32)
        self.ws = torch.empty(_lib.lib.rick_fc_workspace_floats(min(batch, FC_MAX_ROWS), cfg.width, cfg.dim), **f32)
        self._desc = {}

    def _descriptors(self, n):
        """The rick_inc_conv of every GEMM for n prompts (host structures, built once per n)."""
        if n not in self._desc:
            c, d = self.cfg, {}
            rows = n * c.tokens

            def lin(name, k, co, dst):
                _, _, cop, bn = self.gemm[name]
                return gemm_conv.descriptor(rows, 1, 1, k, (1, 1), (1, 1), (0, 0), cop, bn, [(dst.data_ptr(), co, 0, co)])

            for i in range(c.layers):
                b = f'blocks.{i}.'
                d[b + 'qkv'] = lin(b + 'qkv', c.width, 3 * c.width, self.qkv)
                d[b + 'out'] = lin(b + 'out', c.width, c.width, self.tok)
                d[b + 'fc'] = lin(b + 'fc', c.width, c.mlp, self.hid)
                d[b + 'proj'] = lin(b + 'proj', c.mlp, c.width, self.tok)
            self._desc[n] = d
        return self._desc[n]

    def upload(self, ids):
        """ids [n, T] int64 CPU, validated -> the device's id block: the ids, then row n' T + eot(n') of every prompt."""
        n, T = ids.shape
        eot = check_rows(torch.arange(n) * T + eot_positions(ids), n * T)
        self.ids[:n * T + n].copy_(torch.cat([ids.reshape(-1).to(torch.int32), eot]))

    def run(self, n, out):
        """The n prompts of the last upload -> out [n, D] (contiguous rows)."""
        L, c = self._lib, self.cfg
        lib, stream = L.lib, L.stream_ptr()
        rows, d, v = n * c.tokens, self._descriptors(n), self.vec
        eot_ptr = self.ids.data_ptr() + 4 * rows

        def gemm(name, src, res=None, act=0):
            wpk, bias, _, _ = self.gemm[name]
            L.check(lib.rick_inc_conv_lin_f32(src.data_ptr(), wpk.data_ptr(), bias.data_ptr(), None if res is None else res.data_ptr(),
                                              act, d[name], stream), 'rick_inc_conv_lin_f32')

        def layernorm(name, src, dst):
            L.check(lib.rick_clip_layernorm_f32(src.data_ptr(), c.width, v[name + '.w'].data_ptr(), v[name + '.b'].data_ptr(),
                                                dst.data_ptr(), rows, c.width, EPS, stream), 'rick_clip_layernorm_f32')

        L.check(lib.rick_clip_text_tokens_f32(self.ids.data_ptr(), v['tok'].data_ptr(), v['pos'].data_ptr(), self.tok.data_ptr(), n,
                                              c.tokens, c.vocab, c.width, stream), 'rick_clip_text_tokens_f32')
        for i in range(c.layers):
            b = f'blocks.{i}.'
            layernorm(b + 'ln1', self.tok, self.ln)
            gemm(b + 'qkv', self.ln)
            L.check(lib.rick_clip_attention_causal_f32(self.qkv.data_ptr(), self.att.data_ptr(), n, c.tokens, c.heads, c.width // c.heads,
                                                       stream), 'rick_clip_attention_causal_f32')
            gemm(b + 'out', self.att, res=self.tok)           # the residual in place
            layernorm(b + 'ln2', self.tok, self.ln)
            gemm(b + 'fc', self.ln, act=1)
            gemm(b + 'proj', self.hid, res=self.tok)
        L.check(lib.rick_clip_layernorm_rows_f32(self.tok.data_ptr(), eot_ptr, v['ln_final.w'].data_ptr(), v['ln_final.b'].data_ptr(),
                                                 self.post.data_ptr(), n, c.width, EPS, stream), 'rick_clip_layernorm_rows_f32')
        run_fc(self.post.data_ptr(), self.head.data_ptr(), self.head_bias.data_ptr(), self.ws.data_ptr(), out.data_ptr(), n, c.width,
               c.dim, 0)


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
