"""Independent fp64 restatement of DINOv2's ViT, written from the specification (one image at a time, explicit index arithmetic
and matrix products, no torch.nn.functional network ops):

1. bicubic resize to S x S by F.interpolate's rule (tests/clip_f64.py), then (x * 0.5 + 0.5 - mean_c) / std_c with ImageNet's
   constants;
2. P x P stride-P patches in row-major order times the patch filter, plus its bias; [cls ; patches] + pos, the positional
   embedding brought from the checkpoint's g x g grid to (S / P)^2 by the same written bicubic rule on the patch rows (the
   class row kept; nothing done when the grids agree);
3. L blocks: t += ls1 * out(attention(norm1 t)); t += ls2 * fc2(gelu(fc1(norm2 t))), gelu(u) = 0.5 u (1 + erf(u / sqrt 2)),
   LayerNorm eps 1e-6, biased variance; head h owns columns [h d, (h + 1) d): softmax(q k^T / sqrt(d)) v;
4. the final LayerNorm on token 0.

It reads a state_dict in the transformers layout.  Plus synthetic weights in both layouts and GEMM-epilogue helpers.  Nothing
here imports rick_amd.dinov2."""
import math

import torch

from tests.clip_f64 import SmoothG, bicubic_f64, clip_images, cubic_taps, max_rel_err  # noqa: F401  (re-exported)

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def affine_f64(x, mean=MEAN, std=STD):
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (mean, std))
    return (x.double() * 0.5 + 0.5 - mean) / std


def gelu_f64(u):
    return 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))


def pos_f64(pos, grid):
    """pos [g^2 + 1, Wd] fp64 -> [grid^2 + 1, Wd]: the patch rows as a g x g image of Wd channels, resized by the bicubic rule."""
    g, wd = math.isqrt(pos.shape[0] - 1), pos.shape[1]
    if g == grid:
        return pos
    iy, wy = cubic_taps(g, grid)
    img = pos[1:].reshape(g, g, wd)
    rows = (img[:, iy] * wy[None, :, :, None]).sum(2)         # [g, grid, Wd]: along x
    out = (rows[iy] * wy[:, :, None, None]).sum(1)            # [grid, grid, Wd]: along y
    return torch.cat([pos[:1], out.reshape(grid * grid, wd)])


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-6) * w + b


def features_f64(sd, x, heads, size):
    """x [N, 3, H, W] fp32 -> the normalised class tokens [N, Wd] fp64; sd in the transformers layout."""
    g = lambda k: sd[k].double()                                              # noqa: E731
    conv, cb = g('embeddings.patch_embeddings.projection.weight'), g('embeddings.patch_embeddings.projection.bias')
    wd, _, P, _ = conv.shape
    G = size // P
    pos = pos_f64(g('embeddings.position_embeddings')[0], G)
    layers = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith('encoder.layer.'))
    d = wd // heads
    img = affine_f64(bicubic_f64(x, size))
    out = []
    for im in img:
        patches = im.reshape(3, G, P, G, P).permute(1, 3, 0, 2, 4).reshape(G * G, 3 * P * P)      # row-major patches, (c, ky, kx)
        t = torch.cat([g('embeddings.cls_token')[0], patches @ conv.reshape(wd, -1).T + cb]) + pos
        for i in range(layers):
            pre = f'encoder.layer.{i}.'
            lin = lambda v, name: v @ g(pre + name + '.weight').T + g(pre + name + '.bias')      # noqa: E731
            h = _ln(t, g(pre + 'norm1.weight'), g(pre + 'norm1.bias'))
            q, k, v = (lin(h, f'attention.attention.{n}') for n in ('query', 'key', 'value'))
            att = torch.empty_like(q)
            for hd in range(heads):
                c = slice(hd * d, (hd + 1) * d)
                s = q[:, c] @ k[:, c].T / math.sqrt(d)
                e = torch.exp(s - s.max(1, keepdim=True).values)
                att[:, c] = (e / e.sum(1, keepdim=True)) @ v[:, c]
            t = t + g(pre + 'layer_scale1.lambda1') * lin(att, 'attention.output.dense')
            u = lin(_ln(t, g(pre + 'norm2.weight'), g(pre + 'norm2.bias')), 'mlp.fc1')
            t = t + g(pre + 'layer_scale2.lambda1') * lin(gelu_f64(u), 'mlp.fc2')
        out.append(_ln(t[0], g('layernorm.weight'), g('layernorm.bias')))
    return torch.stack(out)


# ---- synthetic weights ----------------------------------------------------------------------------------------------------
def synthetic_dinov2_state_dict(cfg, seed, layout='transformers'):
    """cfg: dict(width, patch, image, layers, mlp).  The same seeded fp32 weights in the 'transformers' layout ('transformers-
    prefixed': under dinov2., with a classifier beside it) or the 'original' one.  Fan-in-scaled normals keep the residual
    stream O(1); LayerNorm weights are spread around 1, LayerScale over [0.5, 1], and every bias is non-zero."""
    wd, P, L, M = cfg['width'], cfg['patch'], cfg['layers'], cfg['mlp']
    T = (cfg['image'] // P) ** 2 + 1
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: torch.randn(*s, generator=gen) * std            # noqa: E731
    lnw = lambda: 1 + 0.2 * rn(wd)                                            # noqa: E731
    ls = lambda: 0.5 + 0.5 * torch.rand(wd, generator=gen)                    # noqa: E731
    hf = layout != 'original'
    pre = 'dinov2.' if layout == 'transformers-prefixed' else ''
    names = (('embeddings.patch_embeddings.projection', 'embeddings.cls_token', 'embeddings.position_embeddings', 'layernorm',
              'embeddings.mask_token') if hf else ('patch_embed.proj', 'cls_token', 'pos_embed', 'norm', 'mask_token'))
    sd = {pre + names[0] + '.weight': rn(wd, 3, P, P, std=(3 * P * P) ** -0.5), pre + names[0] + '.bias': rn(wd, std=0.1),
          pre + names[1]: rn(1, 1, wd, std=0.5), pre + names[2]: rn(1, T, wd, std=0.3), pre + names[4]: rn(1, wd)}
    for i in range(L):
        qkv_w, qkv_b = rn(3 * wd, wd, std=wd ** -0.5), rn(3 * wd, std=0.1)
        ln1, ln2, ls1, ls2 = (lnw(), rn(wd, std=0.1)), (lnw(), rn(wd, std=0.1)), ls(), ls()
        out, fc, proj = (rn(wd, wd, std=wd ** -0.5), rn(wd, std=0.05)), (rn(M, wd, std=wd ** -0.5), rn(M, std=0.1)), \
            (rn(wd, M, std=M ** -0.5), rn(wd, std=0.05))
        if hf:
            b = f'{pre}encoder.layer.{i}.'
            for j, n in enumerate(('query', 'key', 'value')):
                sd[f'{b}attention.attention.{n}.weight'] = qkv_w[j * wd:(j + 1) * wd].clone()
                sd[f'{b}attention.attention.{n}.bias'] = qkv_b[j * wd:(j + 1) * wd].clone()
            sd[b + 'layer_scale1.lambda1'], sd[b + 'layer_scale2.lambda1'] = ls1, ls2
            table = (('norm1', ln1), ('attention.output.dense', out), ('norm2', ln2), ('mlp.fc1', fc), ('mlp.fc2', proj))
        else:
            b = f'blocks.{i}.'
            sd[b + 'attn.qkv.weight'], sd[b + 'attn.qkv.bias'] = qkv_w, qkv_b
            sd[b + 'ls1.gamma'], sd[b + 'ls2.gamma'] = ls1, ls2
            table = (('norm1', ln1), ('attn.proj', out), ('norm2', ln2), ('mlp.fc1', fc), ('mlp.fc2', proj))
        for name, (w, bias) in table:
            sd[f'{b}{name}.weight'], sd[f'{b}{name}.bias'] = w, bias
    sd[pre + names[3] + '.weight'], sd[pre + names[3] + '.bias'] = lnw(), rn(wd, std=0.1)
    if pre:
        sd['classifier.weight'], sd['classifier.bias'] = rn(10, 2 * wd), rn(10)
    return sd
