"""Hand-written fp64 adjoints of the CLIP image tower's stages with respect to the data, written from the formulas (no
autograd inside them) and independently of rick_amd: QuickGELU's derivative, LayerNorm's data gradient, the token / ln_pre
adjoint, attention's backward pass, the adjoint of the bicubic input with the affine, and the two CLIP-space loss heads.
tests/test_clip_grad.py holds them to torch fp64 autograd of the forward restatement (tests/clip_f64.py).

Plus the shared inputs of the gradient tests and the fp32 torch CPU autograd compositions whose error against fp64 is the
base figure of every device bound (the rule of tests/test_gpu_clip.py); `python -m tests.clip_grad_f64` prints them all."""
import math

import torch
import torch.nn.functional as F

from tests.clip_f64 import MEAN, STD, affine_f64, bicubic_f64, cubic_taps, max_rel_err


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the adjoints -----------------------------------------------------------------------------------------------------------
def quickgelu_grad_f64(u, g):
    u, g = u.double(), g.double()
    s = 1 / (1 + torch.exp(-1.702 * u))
    return g * (s + 1.702 * u * s * (1 - s))


def layernorm_grad_f64(x, w, g, eps=1e-5):
    """d/dx of sum(g * (LayerNorm(x) w + b)) over the last axis' rows."""
    x, gw = x.double(), g.double() * w.double()
    mu = x.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mu) * rstd
    return rstd * (gw - gw.mean(-1, keepdim=True) - xh * (gw * xh).mean(-1, keepdim=True))


def tokens_grad_f64(patches, pos, w, g):
    """patches [N, T - 1, C], pos [T, C], g [N, T, C] -> [N, T - 1, C]: ln_pre's gradient on the patch rows."""
    return layernorm_grad_f64(patches.double() + pos.double()[1:], w, g[:, 1:])


def attention_grad_f64(qkv, go, d, heads):
    """qkv [n, T, 3 Wd], go [n, T, Wd] -> the gradient [n, T, 3 Wd] of sum(go * attention(qkv))."""
    n, T, _ = qkv.shape
    split = lambda u: u.reshape(n, T, heads, d).transpose(1, 2)                  # noqa: E731  [n, heads, T, d]
    q, k, v = (split(u) for u in qkv.double().reshape(n, T, 3, heads * d).unbind(2))
    g = split(go.double())
    scale = 1 / math.sqrt(d)
    s = q @ k.transpose(2, 3) * scale
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    dp = g @ v.transpose(2, 3)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    parts = [ds @ k * scale, ds.transpose(2, 3) @ q * scale, p.transpose(2, 3) @ g]
    return torch.stack([u.transpose(1, 2).reshape(n, T, heads * d) for u in parts], 2).reshape(n, T, 3 * heads * d)


def _axis_matrix(n_in, n_out):
    """[n_out, n_in] fp64: the bicubic resize of one axis as a matrix (taps clamped onto a border pixel add up)."""
    idx, w = cubic_taps(n_in, n_out)
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    m.scatter_add_(1, idx, w)
    return m


def input_grad_f64(g, H, W):
    """g [N, 3, S, S], the gradient with respect to affine(bicubic(x)) -> [N, 3, H, W]."""
    S = g.shape[-1]
    g = g.double() * 0.5 / torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    return _axis_matrix(H, S).T @ g @ _axis_matrix(W, S)


def patch_rows(g, P):
    """g [N, 3, S, S] -> the patch-row layout [N G^2, P P 4] of the patch embedding's data gradient: rows (n, gy, gx) in
    row-major order, columns (ky, kx, c) with a fourth channel (given the value 7: the adjoint must ignore it)."""
    N, _, S, _ = g.shape
    G = S // P
    g4 = torch.cat([g, torch.full_like(g[:, :1], 7.0)], 1)
    return g4.reshape(N, 4, G, P, G, P).permute(0, 2, 4, 3, 5, 1).reshape(N * G * G, P * P * 4).contiguous()


def _unit(x):
    return x / x.norm(dim=-1, keepdim=True)


def _cos(a, b, eps=1e-8):
    return (a * b).sum(-1) / (a.norm(dim=-1).clamp_min(eps) * b.norm(dim=-1).clamp_min(eps))


def directional_loss_f64(e_t, e_s, direction):
    e_t, e_s, direction = e_t.double(), e_s.double(), direction.double()
    return (1 - _cos(_unit(e_t) - _unit(e_s), direction[None])).mean()


def within_loss_f64(e_t, e_s):
    t, s = _unit(e_t.double()), _unit(e_s.double())
    terms = [1 - _cos(s[i] - s[j], t[i] - t[j]) for i in range(len(t)) for j in range(i + 1, len(t))]
    return torch.stack(terms).mean()


def domain_direction_f64(emb_source, emb_target):
    return _unit(_unit(emb_target.double()).mean(0) - _unit(emb_source.double()).mean(0))


# ---- shared inputs and the fp32 CPU autograd compositions -------------------------------------------------------------------
def layernorm_bwd_inputs(R, C, offset=False):
    """x, w, g; offset: rows with mean 100 and standard deviation 1."""
    gen = _gen(R * 10000 + C + 5)
    x = torch.randn(R, C, generator=gen)
    x = x + 100 if offset else x * 1.5 + 0.3
    return x, 1 + 0.2 * torch.randn(C, generator=gen), torch.randn(R, C, generator=gen)


def layernorm_bwd_cpu(x, w, g):
    x = x.clone().requires_grad_()
    F.layer_norm(x, (x.shape[-1],), w, torch.zeros_like(w), 1e-5).backward(g)
    return x.grad


def quickgelu_bwd_inputs():
    gen = _gen(51)
    return torch.randn(51, 192, generator=gen) * 3, torch.randn(51, 192, generator=gen)


def quickgelu_bwd_cpu(u, g):
    u = u.clone().requires_grad_()
    (u * torch.sigmoid(1.702 * u)).backward(g)
    return u.grad


def attention_bwd_inputs(T, d, heads, qscale=1.0):
    gen = _gen(T * 100 + d + 7)
    qkv = torch.randn(3, T, 3, heads * d, generator=gen)
    qkv[:, :, 0] *= qscale
    return qkv.reshape(3, T, 3 * heads * d).contiguous(), torch.randn(3, T, heads * d, generator=gen)


def attention_bwd_cpu(qkv, go, d, heads):
    n, T, _ = qkv.shape
    x = qkv.clone().requires_grad_()
    q, k, v = (u.reshape(n, T, heads, d).transpose(1, 2) for u in x.reshape(n, T, 3, heads * d).unbind(2))
    out = (torch.softmax(q @ k.transpose(2, 3) / math.sqrt(d), -1) @ v).transpose(1, 2).reshape(n, T, heads * d)
    out.backward(go)
    return x.grad


def tokens_bwd_inputs():
    gen = _gen(78)
    N, T, C = 3, 17, 64
    return (torch.randn(N, T - 1, C, generator=gen), torch.randn(T, C, generator=gen), 1 + 0.2 * torch.randn(C, generator=gen),
            torch.randn(N, T, C, generator=gen))


def tokens_bwd_cpu(patches, pos, w, g):
    return layernorm_bwd_cpu(patches + pos[1:], w, g[:, 1:])


def input_bwd_inputs(S=224):
    """The upstream gradient [2, 3, S, S] (two images, as tests/test_gpu_clip.py's input_images)."""
    return torch.randn(2, 3, S, S, generator=_gen(S))


def input_bwd_cpu(g, H, W):
    x = torch.zeros(g.shape[0], 3, H, W, requires_grad=True)
    y = F.interpolate(x, size=g.shape[-2:], mode='bicubic', align_corners=False)
    mean, std = (torch.tensor(v).view(1, 3, 1, 1) for v in (MEAN, STD))
    ((y * 0.5 + 0.5 - mean) / std).backward(g)
    return x.grad


def input_bwd_autograd_f64(g, H, W):
    x = torch.zeros(g.shape[0], 3, H, W, dtype=torch.float64, requires_grad=True)
    affine_f64(bicubic_f64(x, g.shape[-1])).backward(g.double())
    return x.grad


def network_upstream(n, dim, seed=3):
    return torch.randn(n, dim, generator=_gen(seed))


def measure():
    """Every base figure the GPU tests quote: fp32 torch CPU autograd against fp64 on the shared inputs."""
    from rick_amd.clip import ClipImageFeatures
    from tests.clip_f64 import embed_f64, synthetic_clip_state_dict
    from tests.test_gpu_clip import CONFIGS, network_inputs
    u, g = quickgelu_bwd_inputs()
    print(f'QGELU_BWD_CPU_BASE = {max_rel_err(quickgelu_bwd_cpu(u, g), quickgelu_grad_f64(u, g)):.3e}')
    for R, C in ((51, 64), (5, 36), (3, 1024), (51, 768)):
        x, w, g = layernorm_bwd_inputs(R, C)
        print(f'LN_BWD ({R}, {C}): {max_rel_err(layernorm_bwd_cpu(x, w, g), layernorm_grad_f64(x, w, g)):.3e}')
    x, w, g = layernorm_bwd_inputs(51, 64)
    print(f'LN_BWD strided: {max_rel_err(layernorm_bwd_cpu(x[::17], w, g[::17]), layernorm_grad_f64(x[::17], w, g[::17])):.3e}')
    x, w, g = layernorm_bwd_inputs(51, 768, offset=True)
    print(f'LN_BWD offset: {max_rel_err(layernorm_bwd_cpu(x, w, g), layernorm_grad_f64(x, w, g)):.3e}')
    for T, d, heads in ((17, 16, 4), (50, 64, 2), (82, 32, 2), (257, 64, 1)):
        for qs in (1.0, 30.0):
            qkv, go = attention_bwd_inputs(T, d, heads, qs)
            got, ref = attention_bwd_cpu(qkv, go, d, heads), attention_grad_f64(qkv, go, d, heads)
            wd = heads * d
            errs = [max_rel_err(got[..., i * wd:(i + 1) * wd], ref[..., i * wd:(i + 1) * wd]) for i in range(3)]
            print(f'ATT_BWD ({T}, {d}, {heads}) x{qs:g}: dq {errs[0]:.3e} dk {errs[1]:.3e} dv {errs[2]:.3e}')
    t = tokens_bwd_inputs()
    print(f'TOKENS_BWD: {max_rel_err(tokens_bwd_cpu(*t), tokens_grad_f64(*t)):.3e}')
    g = input_bwd_inputs()
    for hw in ((256, 256), (64, 64), (100, 317)):
        print(f'INPUT_BWD {hw}: {max_rel_err(input_bwd_cpu(g, *hw), input_grad_f64(g, *hw)):.3e}')
    for name, size, n in (('A', 32, 3), ('A', 64, 3), ('B', 256, 3), ('A', 32, 8), ('A', 64, 8), ('B', 256, 8)):
        cfg, heads = CONFIGS[name]
        sd = synthetic_clip_state_dict(cfg, 11)
        x = network_inputs(name, size)[:n]
        r = network_upstream(n, cfg['dim'])
        x64 = x.double().requires_grad_()
        (embed_f64(sd, x64, heads) * r.double()).sum().backward()
        x32 = x.clone().requires_grad_()
        (ClipImageFeatures.load(sd, device='cpu', heads=heads).encode(x32) * r).sum().backward()
        zeros = float((x64.grad == 0).double().mean())
        print(f'NET_GRAD ({name!r}, {size}, {n}): {max_rel_err(x32.grad, x64.grad):.3e}  (exact zeros {zeros:.2f})')


if __name__ == '__main__':
    measure()
