"""What CLIP's image tower (rick_amd/clip.py) and text tower (rick_amd/cliptext.py) share: the same L pre-LN transformer blocks
and the projection behind them.  One loader of the blocks from either state-dict layout, one check of the limits the kernels
set, one torch composition of the blocks (the CPU path), and one device object, ``Transformer``, that packs the GEMM operands
and issues the launches of a block:

    ln_1, q/k/v GEMM, attention, out_proj GEMM + residual, ln_2, c_fc GEMM (+ QuickGELU), c_proj GEMM + residual

The towers differ around that: the stem that fills the residual stream, the rows the final LayerNorm reads, and whether the
attention is causal.  What differs inside the blocks is data (the attention entry and the buffers a layer reads and writes),
handed to ``Transformer`` as arguments.  The shared library is imported when a launch is built, not before.

DINOv2's ViT (rick_amd/dinov2.py) is a third tower on the same blocks.  What it changes inside them is data as well: the table
of key names, the LayerNorm eps, the activation (the exact GELU), a LayerScale vector behind either branch and no projection.
The defaults are CLIP's."""
import copy
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from . import gemm_conv
from .fc import FC_MAX_ROWS, check_packed, pack_fc_weight, run_fc
from .netutil import get

EPS = 1e-5
MAX_TOKENS, MAX_WIDTH, HEAD_DIMS = 257, 2048, (16, 32, 64)
CUS = 256                       # compute units of the MI355X
ATTENTION, CAUSAL_ATTENTION = 'rick_clip_attention_f32', 'rick_clip_attention_causal_f32'


@functools.cache
def _lib():
    from . import _lib
    return _lib


# ---- loading --------------------------------------------------------------------------------------------------------------
# A table of block key names: the modules of ln1, out, ln2, fc and proj (each with .weight and .bias); 'qkv', either the three
# modules of q, k and v or the (weight, bias) keys of the fused projection, rows q, k, v; optionally 'ls1' and 'ls2', the keys
# of the LayerScale vectors [Wd] behind the attention and the MLP.
_BLOCK_OPENAI = {'ln1': 'ln_1', 'qkv': ('attn.in_proj_weight', 'attn.in_proj_bias'), 'out': 'attn.out_proj', 'ln2': 'ln_2',
                 'fc': 'mlp.c_fc', 'proj': 'mlp.c_proj'}
_BLOCK_HF = {'ln1': 'layer_norm1', 'qkv': ('self_attn.q_proj', 'self_attn.k_proj', 'self_attn.v_proj'), 'out': 'self_attn.out_proj',
             'ln2': 'layer_norm2', 'fc': 'mlp.fc1', 'proj': 'mlp.fc2'}


def shape(sd, key, who):
    if key not in sd:
        raise RuntimeError(f'{who}: missing key {key!r}')
    return tuple(torch.as_tensor(sd[key]).shape)


def layer_count(keys, prefix, who):
    idx = [int(k[len(prefix):].split('.')[0]) for k in keys if k.startswith(prefix) and k[len(prefix):].split('.')[0].isdigit()]
    if not idx:
        raise RuntimeError(f'{who}: missing key {prefix + "0"!r}...: no transformer layer in the state_dict')
    return max(idx) + 1


def blocks_from_state_dict(sd, prefix, hf, wd, who, block=None):
    """The blocks `prefix`{i}. of width wd under the key names of the table `block` (CLIP's of the transformers (hf) or the
    OpenAI layout unless one is given) -> (their parameters as fp32 CPU tensors under the layout-free names
    blocks.{i}.{ln1,qkv,out,ln2,fc,proj}.{w,b} and, where the table names them, blocks.{i}.{ls1,ls2}; the keys of sd that were
    read).  Separate q, k and v are concatenated into qkv, rows q, k, v."""
    p, used = {}, set()
    block = block or (_BLOCK_HF if hf else _BLOCK_OPENAI)

    def take(key, shape_):
        used.add(key)
        return get(sd, key, shape_, who, (RuntimeError, RuntimeError))

    for i in range(layer_count(sd.keys(), prefix, who)):
        src, dst = f'{prefix}{i}.', f'blocks.{i}.'
        mlp = shape(sd, f'{src}{block["fc"]}.weight', who)[0]
        if len(block['qkv']) == 3:
            parts = [take(f'{src}{proj}.{suffix}', shape_)
                     for suffix, shape_ in (('weight', (wd, wd)), ('bias', (wd,))) for proj in block['qkv']]
            p[dst + 'qkv.w'], p[dst + 'qkv.b'] = torch.cat(parts[:3]).contiguous(), torch.cat(parts[3:]).contiguous()
        else:
            p[dst + 'qkv.w'] = take(src + block['qkv'][0], (3 * wd, wd))
            p[dst + 'qkv.b'] = take(src + block['qkv'][1], (3 * wd,))
        for name, shape_ in (('ln1', None), ('out', (wd, wd)), ('ln2', None), ('fc', (mlp, wd)), ('proj', (wd, mlp))):
            p[f'{dst}{name}.w'] = take(f'{src}{block[name]}.weight', shape_ or (wd,))
            p[f'{dst}{name}.b'] = take(f'{src}{block[name]}.bias', (shape_[0],) if shape_ else (wd,))
        for name in ('ls1', 'ls2'):
            if name in block:
                p[dst + name] = take(src + block[name], (wd,))
    return p, used


def head_from_state_dict(sd, key, hf, wd, who):
    """The projection as [D, Wd]: the transformers layout stores it so, OpenAI's is [Wd, D]."""
    hshape = shape(sd, key, who)
    if len(hshape) != 2 or hshape[1 if hf else 0] != wd:
        raise RuntimeError(f'{who}: key {key!r} has shape {hshape}, expected {"(D, Wd)" if hf else "(Wd, D)"}')
    head = get(sd, key, hshape, who, (RuntimeError, RuntimeError))
    return head if hf else head.t().contiguous()


def refuse_unexpected(sd, used, ignored, who):
    extra = sorted(k for k in sd if k not in used and not ignored(k))
    if extra:
        raise RuntimeError(f'{who}: unexpected key {extra[0]!r} in the state_dict')


def limits(p, wd, tokens, heads, noun, who):
    """(layers, MLP width, heads) of the loaded blocks p; refuses what the kernels do not support.  `noun`: what a row of the
    positional embedding is, for the message."""
    if tokens > MAX_TOKENS:
        raise RuntimeError(f'{who}: {tokens} {noun}, at most {MAX_TOKENS} are supported')
    layers = 1 + max(int(k.split('.')[1]) for k in p if k.startswith('blocks.'))
    mlp = p['blocks.0.fc.w'].shape[0]
    if wd % 4 or mlp % 4 or wd > MAX_WIDTH:
        raise RuntimeError(f'{who}: width {wd} / MLP width {mlp}: multiples of 4 and a width of at most {MAX_WIDTH} are supported')
    if heads is None:
        if wd % 64:
            raise RuntimeError(f'{who}: width {wd} is no multiple of 64 (heads = width / 64 is CLIP\'s rule); pass heads=')
        heads = wd // 64
    if heads < 1 or wd % heads or wd // heads not in HEAD_DIMS:
        raise RuntimeError(f'{who}: width {wd} with {heads} heads: the head dim must be one of {HEAD_DIMS}')
    return layers, mlp, int(heads)


# ---- the blocks as a plain torch composition ------------------------------------------------------------------------------
ACTIVATIONS = ('quickgelu', 'gelu')      # u sigmoid(1.702 u) (CLIP); the exact 0.5 u (1 + erf(u / sqrt 2)) (DINOv2)


def check_activation(act, who):
    if act not in ACTIVATIONS:
        raise RuntimeError(f'{who}: activation {act!r}, expected one of {ACTIVATIONS}')


def layer_scales(p, i):
    """(ls1, ls2) of block i, the LayerScale vectors [Wd] behind its attention and its MLP; None where p has none."""
    return p.get(f'blocks.{i}.ls1'), p.get(f'blocks.{i}.ls2')


def torch_blocks(p, cfg, t, mask=None, eps=EPS, act='quickgelu'):
    """The L blocks on the residual stream t [n, T, Wd], in the dtype and on the device of t and the parameters p; mask: an
    additive [T, T] mask on the attention scores (the text tower's causal one); eps: of the LayerNorms; act: one of
    ACTIVATIONS.  Where p holds blocks.{i}.ls1 / ls2 (LayerScale), the branch is multiplied by it before it joins the stream."""
    check_activation(act, 'torch_blocks')
    wd, d, T = cfg.width, cfg.width // cfg.heads, cfg.tokens
    n = t.shape[0]
    for i in range(cfg.layers):
        b = f'blocks.{i}.'
        ls1, ls2 = layer_scales(p, i)
        h = F.layer_norm(t, (wd,), p[b + 'ln1.w'], p[b + 'ln1.b'], eps)
        q, k, v = (u.view(n, T, cfg.heads, d).transpose(1, 2) for u in F.linear(h, p[b + 'qkv.w'], p[b + 'qkv.b']).split(wd, 2))
        s = q @ k.transpose(2, 3) * (1.0 / math.sqrt(d))
        a = torch.softmax(s if mask is None else s + mask, -1) @ v
        a = F.linear(a.transpose(1, 2).reshape(n, T, wd), p[b + 'out.w'], p[b + 'out.b'])
        t = t + (a if ls1 is None else a * ls1)
        h = F.linear(F.layer_norm(t, (wd,), p[b + 'ln2.w'], p[b + 'ln2.b'], eps), p[b + 'fc.w'], p[b + 'fc.b'])
        h = F.linear(h * torch.sigmoid(1.702 * h) if act == 'quickgelu' else F.gelu(h), p[b + 'proj.w'], p[b + 'proj.b'])
        t = t + (h if ls2 is None else h * ls2)
    return t


# ---- GEMM operands and launches -------------------------------------------------------------------------------------------
def pack_linear(w, b, bn=None):
    """A linear layer W [out, in], b [out] as the 1 x 1 convolution's operand: wpk[k, o] = W[o, k].  (wpk, bias, Cop, bn)."""
    return gemm_conv.pack(w[:, :, None, None], b, bn=bn)


def column_block(co, rows):
    """gemm_conv.column_block(co), but 64 where 128-column blocks on `rows` GEMM rows (a full batch) would leave some of the
    256 CUs without a block: the kernel's tiles are 128 rows tall, there is no split-K, and a block's time is set by K.  The
    sums, and so the bits, do not depend on the block."""
    bn = gemm_conv.column_block(co)
    return 64 if bn == 128 and -(-rows // 128) * (co // 128) < CUS else bn


def operand(packed, device):
    """A packed GEMM operand (wpk, bias, Cop, bn) with its tensors on the device."""
    wpk, bias, cop, bn = packed
    return wpk.to(device), bias.to(device), cop, bn


Launch = namedtuple('Launch', 'what fn name args')
Launch.__doc__ = """A kernel launch with its arguments resolved to pointers and numbers, all but the stream: it is built once per
batch size and issued on every call.  what: the launch's place in a block ('ln1', 'qkv', 'attention', 'out', 'ln2', 'fc',
'quickgelu', 'proj') or in a tower; name: the library's entry, fn."""


def launch(what, name, *args):
    return Launch(what, getattr(_lib().lib, name), name, args)


def issue(launches, stream=None):
    """Issues the launches in order, on the current stream unless one is given."""
    L = _lib()
    stream = L.stream_ptr() if stream is None else stream
    for s in launches:
        L.check(s.fn(*s.args, stream), s.name)


def gemm(what, op, a, src, res=None, act=0):
    """dst = act(src * wpk + bias) [+ res] with the destination of the descriptor a: act 1 is QuickGELU, 0 the identity."""
    return launch(what, 'rick_inc_conv_lin_f32', src.data_ptr(), op[0].data_ptr(), op[1].data_ptr(), None if res is None else res.data_ptr(),
                  act, a)


def gemm_vit(what, op, a, src, scale=None, res=None, act=0):
    """dst = act(src * wpk + bias) [* scale] [+ res] on rick_inc_conv_vit_f32: act 1 is the exact GELU, 0 the identity; scale
    [Co] is a LayerScale vector."""
    return launch(what, 'rick_inc_conv_vit_f32', src.data_ptr(), op[0].data_ptr(), op[1].data_ptr(),
                  None if scale is None else scale.data_ptr(), None if res is None else res.data_ptr(), act, a)


def linear(what, op, rows, k, co, src, dst, res=None, act=0, scale=None, vit=False):
    """The GEMM of a linear layer, src [rows, k] -> dst [rows, co], as the 1 x 1 convolution of `rows` one-pixel images; vit: on
    ``gemm_vit`` (its act, its scale) instead of ``gemm``."""
    _, _, cop, bn = op
    a = gemm_conv.descriptor(rows, 1, 1, k, (1, 1), (1, 1), (0, 0), cop, bn, [(dst.data_ptr(), co, 0, co)])
    return gemm_vit(what, op, a, src, scale, res, act) if vit else gemm(what, op, a, src, res, act)


def layernorm(what, w, b, src, ldx, dst, rows, width, eps=EPS):
    """LayerNorm of `rows` rows of src, ldx floats apart, into the contiguous rows of dst."""
    return launch(what, 'rick_clip_layernorm_f32', src.data_ptr(), ldx, w.data_ptr(), b.data_ptr(), dst.data_ptr(), rows, width, eps)


# ---- the blocks and the projection on the device --------------------------------------------------------------------------
class Transformer:
    """The L blocks and the projection for `batch` sequences on the device: per layer the four GEMM operands packed once (the
    column block by ``column_block`` at a full batch), every 1-d parameter and the `tables` of p, the scratch a block reuses
    (LayerNorm output, attention output, the activated hidden layer), the projection's operand, input rows and workspace, and
    a residual stream `tok` and a q|k|v buffer.  `attention` is the attention entry.  `stem`: the sizes in floats of the
    buffers of a tower's stem, allocated here between the operands and the scratch, where the image tower always had them:
    where the buffers lie in device memory moves the time of the GEMMs at 25 images by a percent
    (profiles/r24_bench_clip_refactor.txt).

    A block reads the residual stream in res[2 i], writes it after the attention to res[2 i + 1] and after the MLP to
    res[2 i + 2], and keeps q|k|v in qkv[i].  Without pre, c_fc runs with the fused QuickGELU epilogue; with it, c_fc writes
    the pre-activation to pre[i] with the identity epilogue and rick_clip_quickgelu_f32 follows: the same bits.  A new
    object runs in place, every res `tok` and every qkv the one buffer; ``wired`` gives a view on other buffers.  The
    launches are resolved once per n.

    What else differs between the towers is data too.  `eps` is the LayerNorms'.  `act` is one of ACTIVATIONS, and p may hold
    LayerScale vectors blocks.{i}.{ls1,ls2}: with 'gelu' or a LayerScale the out, fc and proj GEMMs run on
    rick_inc_conv_vit_f32, whose epilogue has the exact GELU and the per-column scale (QuickGELU is not in that epilogue: with
    it, fc stays where it is).  Such a network has no `pre`.  `head`: without a projection p needs no 'head', nothing of the
    projection is built, and the caller's final LayerNorm writes the output rows itself."""

    def __init__(self, p, cfg, batch, device, who, attention, tables=('pos',), stem=(), eps=EPS, act='quickgelu', head=True):
        check_activation(act, who)
        self.cfg, self.batch, self.attention, self.eps, self.act = cfg, batch, attention, eps, act
        self.vit = act == 'gelu' or any(v is not None for i in range(cfg.layers) for v in layer_scales(p, i))
        rows = batch * cfg.tokens
        self.vec = {k: v.to(device) for k, v in p.items() if v.dim() == 1 or k in tables}

        def packed(name):
            w = p[name + '.w']
            return operand(pack_linear(w, p[name + '.b'], column_block(w.shape[0], rows)), device)

        self.gemm = [{name: packed(f'blocks.{i}.{name}') for name in ('qkv', 'out', 'fc', 'proj')} for i in range(cfg.layers)]
        buf = lambda n: torch.empty(n, device=device, dtype=torch.float32)        # noqa: E731
        if head:
            packed_head = pack_fc_weight(p['head'])
            check_packed(packed_head, cfg.width, cfg.dim, who)
            self.head, self.head_bias = packed_head.to(device), torch.zeros(cfg.dim, device=device, dtype=torch.float32)
        self.stem = [buf(n) for n in stem]
        self.tok, self.ln, self.att = (buf(rows * cfg.width) for _ in range(3))
        self.qkv, self.hid = buf(rows * 3 * cfg.width), buf(rows * cfg.mlp)
        if head:
            self.post, self.ws = buf(batch * cfg.width), buf(fc_workspace(batch, cfg.width, cfg.dim))
        self.res, self.qkvs, self.pre, self._launches = [self.tok] * (2 * cfg.layers + 1), [self.qkv] * cfg.layers, None, {}

    def wired(self, res, qkv, pre=None):
        """This object on other buffers per layer (see the class): the same operands, scratch and projection, its own launches."""
        if pre is not None and self.vit:
            raise RuntimeError('Transformer: a kept pre-activation needs the QuickGELU kernel; there is none for GELU or LayerScale')
        other = copy.copy(self)
        other.res, other.qkvs, other.pre, other._launches = res, qkv, pre, {}
        return other

    def layernorm(self, what, name, src, ldx, dst, rows):
        return layernorm(what, self.vec[name + '.w'], self.vec[name + '.b'], src, ldx, dst, rows, self.cfg.width, self.eps)

    def launches(self, n):
        """The launches of the L blocks for n sequences, in order."""
        if n not in self._launches:
            c, out = self.cfg, []
            rows, wd = n * c.tokens, c.width
            for i, op in enumerate(self.gemm):
                (t0, t1, t2), qkv, b = self.res[2 * i:2 * i + 3], self.qkvs[i], f'blocks.{i}.'
                ls1, ls2 = layer_scales(self.vec, i)
                out += [self.layernorm('ln1', b + 'ln1', t0, wd, self.ln, rows),
                        linear('qkv', op['qkv'], rows, wd, 3 * wd, self.ln, qkv),
                        launch('attention', self.attention, qkv.data_ptr(), self.att.data_ptr(), n, c.tokens, c.heads, wd // c.heads),
                        linear('out', op['out'], rows, wd, wd, self.att, t1, res=t0, scale=ls1, vit=self.vit),
                        self.layernorm('ln2', b + 'ln2', t1, wd, self.ln, rows)]
                if self.pre is None:
                    out.append(linear('fc', op['fc'], rows, wd, c.mlp, self.ln, self.hid, act=1, vit=self.act == 'gelu'))
                else:
                    out += [linear('fc', op['fc'], rows, wd, c.mlp, self.ln, self.pre[i]),              # the pre-activation, kept
                            launch('quickgelu', 'rick_clip_quickgelu_f32', self.pre[i].data_ptr(), self.hid.data_ptr(), rows * c.mlp)]
                out.append(linear('proj', op['proj'], rows, c.mlp, wd, self.hid, t2, res=t1, scale=ls2, vit=self.vit))
            self._launches[n] = out
        return self._launches[n]

    def project(self, n, out):
        """The n rows of `post` through the projection -> out [n, D] (contiguous rows)."""
        c = self.cfg
        run_fc(self.post.data_ptr(), self.head.data_ptr(), self.head_bias.data_ptr(), self.ws.data_ptr(), out.data_ptr(), n, c.width, c.dim, 0)


def fc_workspace(batch, k, n):
    """The floats of workspace rick_fc_f32 needs for `batch` rows of a [n, k] layer (fc.run_fc chunks the rows)."""
    return _lib().lib.rick_fc_workspace_floats(min(batch, FC_MAX_ROWS), k, n)
