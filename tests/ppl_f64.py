"""Independent restatement of the perceptual path length (helper, not collected), written from the definitions in
rick_amd/ppl.py's docstring: lerp, slerp, the 1st / 99th percentile filter and the whole metric, the latter composed from the
oracle's generator (oracle/model_ref.py) and the LPIPS definitions of tests/lpips_f64.py.  Every function takes a ``dtype``:
float64 is the reference, float32 is "the fp32 torch composition" whose own deviation from fp64 is the tests' yardstick."""
import math

import torch
import torch.nn.functional as F

from oracle.model_ref import generator_ref, mapping_ref
from tests.lpips_f64 import CONVS, POOL_AT, TAP_AT, _slice

N_MLP = 2


def normalize(x):
    """F.normalize written out: x / max(|x|, 1e-12) over the last dimension."""
    return x / x.pow(2).sum(-1, keepdim=True).sqrt().clamp_min(1e-12)


def lerp(a, b, t):
    return a + (b - a) * t


def slerp(a, b, t):
    an, bn = normalize(a), normalize(b)
    d = (an * bn).sum(-1, keepdim=True).clamp(-1, 1)
    p = t * torch.acos(d)
    c = normalize(bn - d * an)
    return normalize(an * torch.cos(p) + c * torch.sin(p))


def path_latents(a, b, t, eps, space, dtype=torch.float64):
    """[2B, L] in ``dtype``: row 2i the point at t[i], row 2i + 1 the point at t[i] + eps (the sum formed in ``dtype``)."""
    a, b, t = a.to(dtype), b.to(dtype), t.to(dtype)[:, None]
    fn = lerp if space == 'w' else slerp
    return torch.stack([fn(a, b, t), fn(a, b, t + eps)], 1).reshape(2 * a.shape[0], a.shape[1])


def filtered_mean(d):
    """d: a sequence of floats -> the mean of those between the 1st percentile ('lower') and the 99th ('higher'), ends included.
    The k-th percentile of n sorted values sits at the real index (n - 1) k / 100; 'lower' / 'higher' take the sorted value
    below / above it.  Exact integer arithmetic; the sum is math.fsum, the correctly rounded one."""
    s = sorted(float(v) for v in d)
    n = len(s)
    lo, hi = s[(n - 1) * 1 // 100], s[-(-(n - 1) * 99 // 100)]
    keep = [v for v in s if lo <= v <= hi]
    return math.fsum(keep) / len(keep)


def taps(sd, x, dtype):
    """tests/lpips_f64.taps_f64 in ``dtype``."""
    shift = torch.tensor([-.030, -.088, -.188], dtype=dtype).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], dtype=dtype).view(1, 3, 1, 1)
    h = (x.to(dtype) - shift) / scale
    weights = {idx: (sd[f'net.slice{_slice(idx)}.{idx}.weight'].to(dtype), sd[f'net.slice{_slice(idx)}.{idx}.bias'].to(dtype))
               for idx, _, _ in CONVS}
    out = []
    for i in range(30):
        if i in weights:
            h = F.conv2d(h, weights[i][0], weights[i][1], 1, 1)
        elif i in POOL_AT:
            h = F.max_pool2d(h, 2, 2)
        else:
            h = torch.relu(h)
        if i in TAP_AT:
            out.append(h)
    return out


def lpips_rows(sd, img, dtype):
    """LPIPS between rows 2i and 2i + 1 of img [2B, 3, H, W] -> [B] in ``dtype``."""
    val = 0
    for k, f in enumerate(taps(sd, img, dtype)):
        f = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        w = sd[f'lin{k}.model.1.weight'].to(dtype).view(1, -1, 1, 1)
        val = val + ((f[0::2] - f[1::2]) ** 2 * w).sum(1).mean((1, 2))
    return val


def path_distances(sg, sl, size, z0, z1, t, noise, eps, space, crop, dtype=torch.float64):
    """The n per-path distances LPIPS(img(t), img(t + eps)) / eps^2 in ``dtype``, all paths in one batch (the restatement is
    batch-invariant by construction).  sg: generator state_dict, sl: lpips state_dict, noise: per layer [n, 1, r, r]."""
    sg = {k: v.to(dtype) for k, v in sg.items()}
    maps = [m.to(dtype).repeat_interleave(2, 0) for m in noise]
    if space == 'w':
        w = path_latents(mapping_ref(sg, z0.to(dtype), N_MLP), mapping_ref(sg, z1.to(dtype), N_MLP), t, eps, 'w', dtype)
        img, _ = generator_ref(sg, [w], size=size, n_mlp=N_MLP, input_is_latent=True, noise=maps)
    else:
        img, _ = generator_ref(sg, [path_latents(z0, z1, t, eps, 'z', dtype)], size=size, n_mlp=N_MLP, noise=maps)
    if crop:
        c = img.shape[2] // 8
        img = img[:, :, 3 * c:7 * c, 2 * c:6 * c]
    if img.shape[2] > 256:
        img = F.interpolate(img, size=(256, 256), mode='bilinear', align_corners=False)
    return lpips_rows(sl, img, dtype) / (eps * eps)


class RefGenerator(torch.nn.Module):
    """The oracle's functional generator behind rick_amd.models.Generator's interface, in the dtype of its state_dict: what
    the CPU path of perceptual_path_length is given (the HIP generator has no CPU path)."""

    def __init__(self, sg, size, dtype=torch.float32):
        super().__init__()
        self.size, self.style_dim = size, 512
        self.sg = {k: v.to(dtype) for k, v in sg.items()}
        self.anchor = torch.nn.Parameter(torch.zeros(1, dtype=dtype))

    def get_latent(self, z):
        return mapping_ref(self.sg, z, N_MLP)

    def forward(self, styles, input_is_latent=False, noise=None):
        return generator_ref(self.sg, styles, size=self.size, n_mlp=N_MLP, input_is_latent=input_is_latent, noise=noise)


def pinned_paths(n, size, seed, sampling='full'):
    """Fixed (z0, z1, t) and per-layer noise [n, 1, r, r] for n paths of a size x size generator."""
    g = torch.Generator().manual_seed(seed)
    z0, z1 = torch.randn(n, 512, generator=g), torch.randn(n, 512, generator=g)
    t = torch.rand(n, generator=g) if sampling == 'full' else torch.zeros(n)
    sizes = [4] + [2 ** i for i in range(3, int(math.log2(size)) + 1) for _ in range(2)]
    return (z0, z1, t), [torch.randn(n, 1, r, r, generator=g) for r in sizes]
