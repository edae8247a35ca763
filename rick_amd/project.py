"""Projection of target images into the latent space of a generator (W or W+), in the manner of stylegan2-pytorch's
``projector.py``, with the engine's differentiable LPIPS (rick_amd/lpips.py: ``LPIPS.loss``) as the perceptual loss.

    net = LPIPS.load('lpips_vgg.pt', device='cuda', batch=1)
    latent, images, losses = project(g_ema, target, net, steps=1000, rng=torch.Generator().manual_seed(0))

Every step is one generator forward / backward (with respect to the latent only) and one VGG16 forward / backward (with
respect to the image only), all on the HIP kernels; the optimiser state is a few kilobytes and is stepped with torch
elementwise operations.
"""
import math

import torch
import torch.nn.functional as F


def learning_rate(t, lr, rampup=0.05, rampdown=0.25):
    """The projector's schedule at t = step / steps: a linear ramp up over the first ``rampup``, a cosine ramp down over the
    last ``rampdown``."""
    ramp = min(1.0, (1.0 - t) / rampdown)
    ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
    return lr * ramp * min(1.0, t / rampup)


def _randn(shape, rng, device):
    if rng is None:
        return torch.randn(shape, device=device)
    return torch.randn(shape, generator=rng, device=rng.device).to(device)


def latent_statistics(generator, n, rng=None, chunk=10000):
    """Mean [style_dim] and the scalar spread sqrt(sum |w - mean|^2 / n) of the mapping network's output over n draws of z."""
    dev = next(generator.parameters()).device
    with torch.no_grad():
        w = torch.cat([generator.style(_randn((min(chunk, n - lo), generator.style_dim), rng, dev)) for lo in range(0, n, chunk)])
        mean = w.mean(0)
        std = ((w - mean).pow(2).sum() / n) ** 0.5
    return mean, std


def _pool(img, factor):
    return img if factor == 1 else F.avg_pool2d(img, factor)


def _generate(generator, latent):
    """One generator call per image: the generator's kernels promise no batch invariance (unlike the LPIPS ones), so a batch
    of one is what makes an image, and its latent's gradient, independent of the other targets by construction."""
    return torch.cat([generator([latent[i:i + 1]], input_is_latent=True, randomize_noise=False)[0]
                      for i in range(latent.shape[0])])


def project(generator, target, lpips, steps=1000, lr=0.1, w_plus=False, mse=0.0, n_mean_latent=10000, noise=0.05,
            noise_ramp=0.75, lr_rampup=0.05, lr_rampdown=0.25, rng=None):
    """Optimise one latent per target image so that the generator reproduces it.

    generator: a rick_amd Generator on the device of ``lpips``; its weights are not changed.  target: [N, 3, S, S] fp32 in
    [-1, 1], at the generator's resolution or at the resolution the loss sees.  The loss sees the generated image as it is
    up to the LPIPS size (256-px generators pass straight through); larger generators are average-pooled down by the integer
    factor ``generator.size // lpips.size`` (and so is a full-resolution target).

    The latent starts at the mean of ``n_mean_latent`` mapped draws of z, as [N, style_dim] (W) or, with ``w_plus``, as
    [N, n_latent, style_dim] (one row per layer).  Adam (betas 0.9 / 0.999) steps it with the learning rate
    ``learning_rate(i / steps, lr, lr_rampup, lr_rampdown)``; step i evaluates the generator at the latent plus Gaussian noise
    of strength ``latent_std * noise * max(0, 1 - t / noise_ramp)^2`` drawn from ``rng`` (a torch.Generator; the run is
    reproducible from its seed).  The loss is ``lpips.loss(img, target_features).sum() + mse * sum over images of the mean
    squared error``; every image's terms depend on its own latent only, and the generator runs one image at a time, so
    projecting N targets together gives exactly the latents of projecting each alone (with ``noise=0``; the latent noise of
    a joint run is one draw for all N).

    The generator's per-layer noise is fixed to its stored ``noises`` buffers (``randomize_noise=False``) and is NOT
    optimised, unlike stylegan2-pytorch's projector, which also descends on the noise maps and regularises them.

    Returns (latent, images, losses): the final latent, its images [N, 3, size, size] (image i is
    ``generator([latent[i:i + 1]], input_is_latent=True, randomize_noise=False)``), and the loss of every step [steps], summed
    over the N images (on the device)."""
    if target.dim() != 4 or target.shape[1] != 3 or target.dtype != torch.float32:
        raise RuntimeError(f'project: expected target [N, 3, S, S] float32, got {tuple(target.shape)} {target.dtype}')
    if steps < 1:
        raise ValueError('project: steps must be >= 1')
    dev = next(generator.parameters()).device
    gsize = generator.size
    factor = max(1, gsize // lpips.size)
    seen = gsize // factor
    if gsize % factor:
        raise ValueError(f'project: generator size {gsize} is no multiple of the pooling factor {factor}')
    target = target.to(dev)
    if tuple(target.shape[2:]) == (gsize, gsize):
        target = _pool(target, factor)
    if tuple(target.shape[2:]) != (seen, seen):
        raise RuntimeError(f'project: target is {tuple(target.shape[2:])}, expected {gsize}^2 or {seen}^2')
    target = target.contiguous()
    N = target.shape[0]
    tf = lpips.features(target)
    mean, std = latent_statistics(generator, n_mean_latent, rng)
    latent = mean.detach().clone().unsqueeze(0).repeat(N, 1)
    if w_plus:
        latent = latent.unsqueeze(1).repeat(1, generator.n_latent, 1)
    latent = latent.contiguous().requires_grad_(True)
    m, v = torch.zeros_like(latent), torch.zeros_like(latent)
    b1, b2, eps = 0.9, 0.999, 1e-8
    losses = torch.zeros(steps, device=dev, dtype=torch.float32)
    frozen = [p for p in generator.parameters() if p.requires_grad]
    for p in frozen:
        p.requires_grad_(False)
    try:
        for i in range(steps):
            t = i / steps
            strength = std * (noise * max(0.0, 1.0 - t / noise_ramp) ** 2)
            z = latent + _randn(tuple(latent.shape), rng, dev) * strength if noise > 0 else latent + 0.0
            img = _pool(_generate(generator, z), factor)
            loss = lpips.loss(img, tf).sum()
            if mse:
                loss = loss + mse * (img - target).pow(2).mean((1, 2, 3)).sum()
            g, = torch.autograd.grad(loss, latent)
            losses[i] = loss.detach()
            with torch.no_grad():
                m.mul_(b1).add_(g, alpha=1 - b1)
                v.mul_(b2).addcmul_(g, g, value=1 - b2)
                step = learning_rate(t, lr, lr_rampup, lr_rampdown) / (1 - b1 ** (i + 1))
                latent.addcdiv_(m, (v / (1 - b2 ** (i + 1))).sqrt_().add_(eps), value=-step)
        with torch.no_grad():
            out = latent.detach().clone()
            images = _generate(generator, out)
    finally:
        for p in frozen:
            p.requires_grad_(True)
    return out, images, losses
