"""Independent fp64 restatement of CLIP's ViT image tower, written from the specification (one image at a time, explicit
index arithmetic and matrix products, no torch.nn.functional network ops):

1. bicubic resize to S x S by F.interpolate's rule (align_corners=False): source s = (in / S) * (dst + 0.5) - 0.5, taps
   floor(s) - 1 .. floor(s) + 2 clamped into the image, cubic convolution weights with A = -0.75 at t = s - floor(s), no
   antialiasing, overshoot kept; then (x * 0.5 + 0.5 - mean_c) / std_c;
2. P x P stride-P patches in row-major order times the patch filter (no bias); [class ; patches] + positional embedding;
3. ln_pre (eps 1e-5, biased variance);
4. L blocks: t += out_proj(attention(ln_1 t)); t += c_proj(quickgelu(c_fc(ln_2 t))), quickgelu(u) = u / (1 + exp(-1.702 u));
   head h owns columns [h d, (h + 1) d): softmax(q k^T / sqrt(d)) v;
5. ln_post on token 0, then the projection without bias.

It reads a state_dict in the transformers layout.  Plus synthetic weights in both layouts and the error measure.  Nothing
here imports rick_amd.clip."""
import math

import torch

from tests.vgg_f64 import SmoothG, max_rel_err  # noqa: F401  (re-exported)

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
A = -0.75


# ---- step 1 ---------------------------------------------------------------------------------------------------------------
def cubic_taps(n_in, n_out, dtype=torch.float64):
    """(idx [n_out, 4] int64 clamped source indices, w [n_out, 4] weights) of one axis, the arithmetic in `dtype`."""
    scale = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    s = scale * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5
    fl = s.floor()
    t = s - fl
    near = lambda x: ((A + 2) * x - (A + 3)) * x * x + 1                      # noqa: E731  |x| <= 1
    far = lambda x: ((A * x - 5 * A) * x + 8 * A) * x - 4 * A                # noqa: E731  1 < |x| < 2
    w = torch.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], 1)
    idx = (fl.to(torch.int64)[:, None] + torch.arange(-1, 3)).clamp_(0, n_in - 1)
    return idx, w


def bicubic_f64(x, size, dtype=torch.float64):
    """x [N, 3, H, W] -> [N, 3, size, size] by the rule above, in `dtype`."""
    iy, wy = cubic_taps(x.shape[2], size, dtype)
    ix, wx = cubic_taps(x.shape[3], size, dtype)
    x = x.to(dtype)
    rows = (x[:, :, :, ix] * wx).sum(-1)                      # [N, 3, H, size]
    return (rows[:, :, iy] * wy[:, :, None]).sum(3)           # [N, 3, size, 4, size] summed over the four rows


def affine_f64(x):
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (MEAN, STD))
    return (x.double() * 0.5 + 0.5 - mean) / std


# ---- steps 2 to 5 ---------------------------------------------------------------------------------------------------------
def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def embed_f64(sd, x, heads):
    """x [N, 3, H, W] fp32 -> image embeddings [N, D] fp64; sd in the transformers layout."""
    g = lambda k: sd[k].double()                                              # noqa: E731
    conv = g('vision_model.embeddings.patch_embedding.weight')
    wd, _, P, _ = conv.shape
    pos = g('vision_model.embeddings.position_embedding.weight')
    T = pos.shape[0]
    G = math.isqrt(T - 1)
    layers = 1 + max(int(k.split('.')[3]) for k in sd if k.startswith('vision_model.encoder.layers.'))
    d = wd // heads
    img = affine_f64(bicubic_f64(x, G * P))
    out = []
    for im in img:
        patches = im.reshape(3, G, P, G, P).permute(1, 3, 0, 2, 4).reshape(G * G, 3 * P * P)      # row-major patches, (c, ky, kx)
        t = torch.cat([g('vision_model.embeddings.class_embedding')[None], patches @ conv.reshape(wd, -1).T]) + pos
        t = _ln(t, g('vision_model.pre_layrnorm.weight'), g('vision_model.pre_layrnorm.bias'))
        for i in range(layers):
            pre = f'vision_model.encoder.layers.{i}.'
            lin = lambda v, name: v @ g(pre + name + '.weight').T + g(pre + name + '.bias')      # noqa: E731
            h = _ln(t, g(pre + 'layer_norm1.weight'), g(pre + 'layer_norm1.bias'))
            q, k, v = (lin(h, f'self_attn.{n}_proj') for n in 'qkv')
            att = torch.empty_like(q)
            for hd in range(heads):
                c = slice(hd * d, (hd + 1) * d)
                s = q[:, c] @ k[:, c].T / math.sqrt(d)
                e = torch.exp(s - s.max(1, keepdim=True).values)
                att[:, c] = (e / e.sum(1, keepdim=True)) @ v[:, c]
            t = t + lin(att, 'self_attn.out_proj')
            u = lin(_ln(t, g(pre + 'layer_norm2.weight'), g(pre + 'layer_norm2.bias')), 'mlp.fc1')
            t = t + lin(u / (1 + torch.exp(-1.702 * u)), 'mlp.fc2')
        cls = _ln(t[0], g('vision_model.post_layernorm.weight'), g('vision_model.post_layernorm.bias'))
        out.append(cls @ g('visual_projection.weight').T)
    return torch.stack(out)


# ---- synthetic weights ----------------------------------------------------------------------------------------------------
def synthetic_clip_state_dict(cfg, seed, layout='transformers'):
    """cfg: dict(width, patch, image, layers, mlp, dim).  The same seeded fp32 weights in the 'transformers' or the 'openai'
    layout ('openai-visual': with the visual. prefix).  Fan-in-scaled normals keep the residual stream O(1); LayerNorm weights
    are spread around 1 and every bias is non-zero."""
    wd, P, L, M, D = cfg['width'], cfg['patch'], cfg['layers'], cfg['mlp'], cfg['dim']
    T = (cfg['image'] // P) ** 2 + 1
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: torch.randn(*s, generator=gen) * std            # noqa: E731
    lnw = lambda: 1 + 0.2 * rn(wd)                                            # noqa: E731
    hf = layout == 'transformers'
    pre = '' if layout == 'openai' else 'visual.' if layout == 'openai-visual' else 'vision_model.'
    sd = {}
    names = (('embeddings.patch_embedding.weight', 'embeddings.class_embedding', 'embeddings.position_embedding.weight', 'pre_layrnorm',
              'post_layernorm') if hf else ('conv1.weight', 'class_embedding', 'positional_embedding', 'ln_pre', 'ln_post'))
    sd[pre + names[0]] = rn(wd, 3, P, P, std=(3 * P * P) ** -0.5)
    sd[pre + names[1]] = rn(wd, std=0.5)
    sd[pre + names[2]] = rn(T, wd, std=0.3)
    sd[pre + names[3] + '.weight'], sd[pre + names[3] + '.bias'] = lnw(), rn(wd, std=0.1)
    for i in range(L):
        qkv_w, qkv_b = rn(3 * wd, wd, std=wd ** -0.5), rn(3 * wd, std=0.1)
        ln1, ln2 = (lnw(), rn(wd, std=0.1)), (lnw(), rn(wd, std=0.1))
        out, fc, proj = (rn(wd, wd, std=wd ** -0.5), rn(wd, std=0.05)), (rn(M, wd, std=wd ** -0.5), rn(M, std=0.1)), \
            (rn(wd, M, std=M ** -0.5), rn(wd, std=0.05))
        if hf:
            b = f'{pre}encoder.layers.{i}.'
            for j, n in enumerate('qkv'):
                sd[f'{b}self_attn.{n}_proj.weight'] = qkv_w[j * wd:(j + 1) * wd].clone()
                sd[f'{b}self_attn.{n}_proj.bias'] = qkv_b[j * wd:(j + 1) * wd].clone()
            table = (('layer_norm1', ln1), ('self_attn.out_proj', out), ('layer_norm2', ln2), ('mlp.fc1', fc), ('mlp.fc2', proj))
        else:
            b = f'{pre}transformer.resblocks.{i}.'
            sd[b + 'attn.in_proj_weight'], sd[b + 'attn.in_proj_bias'] = qkv_w, qkv_b
            table = (('ln_1', ln1), ('attn.out_proj', out), ('ln_2', ln2), ('mlp.c_fc', fc), ('mlp.c_proj', proj))
        for name, (w, bias) in table:
            sd[f'{b}{name}.weight'], sd[f'{b}{name}.bias'] = w, bias
    sd[pre + names[4] + '.weight'], sd[pre + names[4] + '.bias'] = lnw(), rn(wd, std=0.1)
    head = rn(D, wd, std=wd ** -0.5)
    if hf:
        sd['visual_projection.weight'] = head
    else:
        sd[pre + 'proj'] = head.t().contiguous()
    return sd


def clip_images(n, size, seed):
    """n smooth images [n, 3, size, size] fp32 in [-1, 1] (low-frequency content plus mild noise, so that a resize matters)."""
    g = torch.Generator().manual_seed(seed)
    low = torch.nn.functional.interpolate(torch.rand(n, 3, 5, 5, generator=g) * 2 - 1, (size, size), mode='bilinear', align_corners=False)
    return (0.85 * low + 0.15 * (torch.rand(n, 3, size, size, generator=g) * 2 - 1)).clamp_(-1, 1).contiguous()
