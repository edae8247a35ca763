"""Perceptual path length (PPL; Karras et al., "A Style-Based Generator Architecture for GANs", and its use in "Analyzing and
Improving the Image Quality of StyleGAN"), as stylegan2-pytorch's ``ppl.py`` computes it, streamed on the device.

    ppl, d = perceptual_path_length(g_ema, net, n_samples=5000, space='w')      # net: a rick_amd.lpips.LPIPS

Definition.  For each of ``n_samples`` paths draw two latents z0, z1 ~ N(0, I) and a position t (``sampling='full'``:
t ~ U[0, 1); ``'end'``: t = 0).  Generate the two images at the path points t and t + eps and take

    d = LPIPS(img(t), img(t + eps)) / eps^2 .

PPL is the mean of the d that lie between the 1st and the 99th percentile of all n_samples values (both ends included).

* ``space='w'``: w0 = mapping(z0), w1 = mapping(z1); the path is the straight line ``w0 + (w1 - w0) t`` (torch.lerp) and the
  images are ``g_ema([w], input_is_latent=True)``.
* ``space='z'``: the path is the great circle through z0 / |z0| and z1 / |z1| (slerp):
  ``an = a / |a|``, ``bn = b / |b|``, ``d = clamp(sum an bn, -1, 1)``, ``p = t acos(d)``, ``c = normalize(bn - d an)``,
  ``point = normalize(an cos p + c sin p)``, where ``normalize`` is ``F.normalize`` (division by ``max(norm, 1e-12)``, so
  a == b gives an and no NaN); the images are ``g_ema([z])``.
* Noise: both images of a path share their noise maps, and every path has its own: per layer one ``[2B, 1, r, r]`` tensor whose
  rows 2i and 2i + 1 are equal.  (stylegan2-pytorch's script, as recalled, draws one map per batch; see PAPERS.md.)
* ``crop=True`` keeps ``img[:, :, 3c:7c, 2c:6c]`` with ``c = H // 8`` (the face crop of the FFHQ configuration).
* Images larger than 256 px are resized with ``F.interpolate(size=(256, 256), mode='bilinear', align_corners=False)``.
* The percentiles follow NumPy: ``lo = np.percentile(d, 1, method='lower')``, ``hi = np.percentile(d, 99, method='higher')``,
  i.e. the sorted values at ``floor`` / ``ceil`` of NumPy's virtual index ``n q + (1 - q) - 1``; the mean of the kept values
  is their correctly rounded fp64 sum (``math.fsum``) over their count.  With fewer than 101 samples the filter keeps everything.

What runs where.  The generator, its mapping network and the LPIPS trunk run on their HIP kernels.  ``path_latents`` is
rick_ppl_latents_f32 (one wave per path, both points from one launch) and the 2B images of a batch go through the trunk once;
``LPIPS.paired`` (rick_lpips_paired_f32) then forms the B distances of rows (2i, 2i + 1) of that one feature set, B pairs of
work instead of the (2B)^2 of ``LPIPS.distances``.  The crop, the resize, the noise draws and the final sort are torch
tensor operations (plumbing; the first two are the identity for an uncropped 256 px generator).  The distances stay on the
device in one buffer (``PathLengthStats``); ``finalize`` sorts a copy of it, so the result does not depend on how the
samples were batched as long as each path's distance does not.  CPU tensors take the fp32 torch composition of the same
formulas throughout.
"""
import math

import torch
import torch.nn.functional as F

SPACES = ('w', 'z')
SAMPLINGS = ('end', 'full')
MAX_LATENT = 1024          # rick_ppl_latents_f32: a wave holds a latent row in registers
RESIZE_TO = 256


def _check_eps(eps, who):
    if not isinstance(eps, (int, float)) or not math.isfinite(eps) or eps <= 0:
        raise ValueError(f'ppl.{who}: eps must be a finite number > 0, got {eps!r}')


def path_latents(a, b, t, eps, space):
    """a, b [B, L] fp32, t [B] fp32 -> [2B, L] fp32: row 2i is the path point at t[i], row 2i + 1 the point at t[i] + eps;
    ``space`` 'w' (lerp) or 'z' (slerp), see the module docstring."""
    if space not in SPACES:
        raise ValueError(f"ppl.path_latents: space must be 'w' or 'z', got {space!r}")
    _check_eps(eps, 'path_latents')
    if a.dim() != 2 or a.shape != b.shape or t.shape != a.shape[:1] or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'ppl.path_latents: a {tuple(a.shape)}, b {tuple(b.shape)}, t {tuple(t.shape)}: need [B, L], [B, L], [B]')
    if any(x.dtype != torch.float32 for x in (a, b, t)) or b.device != a.device or t.device != a.device:
        raise ValueError('ppl.path_latents: a, b and t must be float32 tensors on one device')
    B, L = a.shape
    if a.device.type == 'cpu':
        rows = []
        for tt in (t[:, None], t[:, None] + eps):
            if space == 'w':
                rows.append(a + (b - a) * tt)
            else:
                an, bn = F.normalize(a, dim=-1), F.normalize(b, dim=-1)
                d = (an * bn).sum(-1, keepdim=True).clamp(-1, 1)
                p = tt * torch.acos(d)
                c = F.normalize(bn - d * an, dim=-1)
                rows.append(F.normalize(an * torch.cos(p) + c * torch.sin(p), dim=-1))
        return torch.stack(rows, 1).reshape(2 * B, L)
    if L > MAX_LATENT:
        raise ValueError(f'ppl.path_latents: latent dimension {L} exceeds {MAX_LATENT}')
    from . import _lib
    a, b, t = a.contiguous(), b.contiguous(), t.contiguous()
    out = torch.empty((2 * B, L), device=a.device, dtype=torch.float32)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib.rick_ppl_latents_f32(a.data_ptr(), b.data_ptr(), t.data_ptr(), float(eps), out.data_ptr(), B, L,
                                                 SPACES.index(space), _lib.stream_ptr()), 'rick_ppl_latents_f32')
    return out


def draw_paths(n, latent, sampling, generator=None):
    """-> (z0 [n, latent], z1 [n, latent], t [n]) fp32 on the host: the end points of n paths and the position on each,
    t ~ U[0, 1) for ``sampling='full'``, 0 for ``'end'``."""
    if sampling not in SAMPLINGS:
        raise ValueError(f"ppl.draw_paths: sampling must be 'end' or 'full', got {sampling!r}")
    if n < 1 or latent < 1:
        raise ValueError(f'ppl.draw_paths: n = {n}, latent = {latent}: both must be >= 1')
    dev = generator.device if generator is not None else 'cpu'
    z = torch.randn(2, n, latent, generator=generator, device=dev)
    t = torch.rand(n, generator=generator, device=dev) if sampling == 'full' else torch.zeros(n)
    return z[0].cpu(), z[1].cpu(), t.cpu()


def percentile_indices(n):
    """Indices into the n sorted values of NumPy's 1st percentile with method='lower' and 99th with method='higher': floor and
    ceil of the virtual index n q + (1 - q) - 1 (numpy/lib/function_base.py, _compute_virtual_index with alpha = beta = 1),
    evaluated in the same double arithmetic."""
    def virtual(q):
        return n * q + (1.0 + q * (1.0 - 1.0 - 1.0)) - 1.0
    lo, hi = int(math.floor(virtual(1 / 100))), int(math.ceil(virtual(99 / 100)))
    return min(max(lo, 0), n - 1), min(max(hi, 0), n - 1)


class PathLengthStats:
    """One device buffer of ``n_total`` path distances; ``update`` appends a batch, ``finalize`` -> (ppl, distances)."""

    def __init__(self, n_total, device):
        if n_total < 2:
            raise ValueError(f'ppl.PathLengthStats: {n_total} samples are too few for the 1st / 99th percentile filter (need >= 2)')
        self.n_total, self.count = int(n_total), 0
        self.buf = torch.empty(self.n_total, device=device, dtype=torch.float32)

    def update(self, d):
        if d.dim() != 1 or d.dtype != torch.float32 or self.count + d.shape[0] > self.n_total:
            raise ValueError(f'ppl.PathLengthStats.update: {tuple(d.shape)} {d.dtype} onto {self.count} of {self.n_total}')
        self.buf[self.count:self.count + d.shape[0]] = d
        self.count += d.shape[0]
        return self

    def finalize(self):
        """-> (mean in fp64 of the values d with lo <= d <= hi, the distances [n_total] fp32 in the order they came)."""
        if self.count != self.n_total:
            raise RuntimeError(f'ppl.PathLengthStats.finalize: {self.count} of {self.n_total} distances')
        s, _ = torch.sort(self.buf)
        i_lo, i_hi = percentile_indices(self.n_total)
        keep = s[(s >= s[i_lo]) & (s <= s[i_hi])].cpu().tolist()
        return math.fsum(keep) / len(keep), self.buf       # fsum: the correctly rounded fp64 sum, whatever the order


def _noise_sizes(size):
    return [4] + [2 ** i for i in range(3, int(math.log2(size)) + 1) for _ in range(2)]


@torch.no_grad()
def perceptual_path_length(g_ema, net, n_samples=5000, batch=None, eps=1e-4, space='w', sampling='end', crop=False,
                           latents=None, noise=None, generator=None):
    """-> (ppl, distances [n_samples] fp32 on the generator's device); see the module docstring.

    g_ema: a ``rick_amd.models.Generator`` (anything with ``size``, ``style_dim``, ``get_latent`` and the same call); net: a
    ``rick_amd.lpips.LPIPS`` on the same device.  ``batch`` paths (2 x batch images) per step, default ``net.batch // 2``; the
    last step may be short.  ``latents``: fixed paths ``(z0, z1, t)`` as ``draw_paths`` returns them, else drawn from
    ``generator``.  ``noise``: per generator layer one ``[n_samples, 1, r, r]`` tensor, a map per path, else drawn from
    ``generator`` batch by batch."""
    who = 'ppl.perceptual_path_length'
    if space not in SPACES:
        raise ValueError(f"{who}: space must be 'w' or 'z', got {space!r}")
    if sampling not in SAMPLINGS:
        raise ValueError(f"{who}: sampling must be 'end' or 'full', got {sampling!r}")
    _check_eps(eps, 'perceptual_path_length')
    if n_samples < 2:
        raise ValueError(f'{who}: n_samples = {n_samples} is too small for the 1st / 99th percentile filter (need >= 2)')
    if batch is None:
        batch = net.batch // 2
    if batch < 1:
        raise ValueError(f'{who}: batch must be >= 1 (an LPIPS planned for {net.batch} image(s) cannot hold a pair)')
    dev = next(g_ema.parameters()).device
    if dev != net.device:
        raise ValueError(f'{who}: the generator is on {dev}, the LPIPS network on {net.device}')
    latent, sizes = g_ema.style_dim, _noise_sizes(g_ema.size)
    if latents is None:
        latents = draw_paths(n_samples, latent, sampling, generator)
    z0, z1, t = latents
    if tuple(z0.shape) != (n_samples, latent) or z1.shape != z0.shape or tuple(t.shape) != (n_samples,):
        raise ValueError(f'{who}: latents {tuple(z0.shape)}, {tuple(z1.shape)}, {tuple(t.shape)}: need two [{n_samples}, {latent}] '
                         f'and one [{n_samples}]')
    if noise is not None and (len(noise) != len(sizes)
                              or any(tuple(m.shape) != (n_samples, 1, r, r) for m, r in zip(noise, sizes))):
        raise ValueError(f'{who}: noise must be {len(sizes)} tensors [{n_samples}, 1, r, r] with r = {sizes}')
    stats = PathLengthStats(n_samples, dev)
    ws = net.workspace_features if dev.type == 'cuda' else None
    was_training = g_ema.training
    g_ema.eval()
    for lo in range(0, n_samples, batch):
        hi = min(n_samples, lo + batch)
        a, b, tt = (x[lo:hi].to(dev, torch.float32) for x in (z0, z1, t))
        if noise is not None:
            maps = [m[lo:hi].to(dev, torch.float32) for m in noise]
        else:
            gdev = generator.device if generator is not None else dev
            maps = [torch.randn(hi - lo, 1, r, r, generator=generator, device=gdev).to(dev) for r in sizes]
        maps = [m.repeat_interleave(2, 0) for m in maps]                # rows 2i and 2i + 1 share path i's map
        if space == 'w':
            w = path_latents(g_ema.get_latent(a), g_ema.get_latent(b), tt, eps, 'w')
            img, _ = g_ema([w], input_is_latent=True, noise=maps)
        else:
            img, _ = g_ema([path_latents(a, b, tt, eps, 'z')], noise=maps)
        if crop:
            c = img.shape[2] // 8
            img = img[:, :, 3 * c:7 * c, 2 * c:6 * c]
        if img.shape[2] > RESIZE_TO:
            img = F.interpolate(img, size=(RESIZE_TO, RESIZE_TO), mode='bilinear', align_corners=False)
        img = img.contiguous()
        fits = ws is not None and img.shape[0] <= ws.n and tuple(img.shape[2:]) == ws.size
        f = net.features(img, out=ws if fits else None)
        stats.update(net.paired(f) / (eps * eps))
    if was_training:
        g_ema.train()
    return stats.finalize()
