"""The head of the patch-level discriminator (rick_amd/patchd.py, "Head math") restated literally in fp64 with NumPy slices: one
shifted slice per tap, no convolution routine, no code shared with the module.

    z[n,y,x]    = b + sum_c sum_ky sum_kx (wscale w[c,ky,kx]) X[n,c,y+ky-1,x+kx-1]          (zero outside)
    out         = gain (z > 0 ? z : slope z)
    a           = gain (out > 0 ? 1 : slope)
    gz = g a,   gb = sum gz
    gw[c,ky,kx] = wscale sum_{n,y,x} gz[n,y,x] X[n,c,y+ky-1,x+kx-1]
    gX[n,c,u,v] = wscale sum_{ky,kx} w[c,ky,kx] gz[n,u-ky+1,v-kx+1]
"""
import numpy as np


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=np.float64)


def _padded(x):
    N, C, H, W = x.shape
    xp = np.zeros((N, C, H + 2, W + 2))
    xp[:, :, 1:H + 1, 1:W + 1] = x
    return xp


def head_fwd(x, w, b, wscale, slope=0.2, gain=2 ** 0.5):
    """x [N, C, H, W], w [1, C, 3, 3], b [1] -> out [N, 1, H, W], fp64."""
    x, w, b = _f64(x), _f64(w), _f64(b)
    N, C, H, W = x.shape
    xp = _padded(x)
    z = np.full((N, H, W), float(b.reshape(-1)[0]))
    for ky in range(3):
        for kx in range(3):
            for c in range(C):
                z += (wscale * w[0, c, ky, kx]) * xp[:, c, ky:ky + H, kx:kx + W]
    return (gain * np.where(z > 0, z, slope * z))[:, None]


def head_bwd(x, w, g, out, wscale, slope=0.2, gain=2 ** 0.5):
    """-> gX [N, C, H, W], gw [1, C, 3, 3], gb [1], fp64; the sign comes from `out`."""
    x, w, g, out = _f64(x), _f64(w), _f64(g), _f64(out)
    N, C, H, W = x.shape
    gz = g[:, 0] * (gain * np.where(out[:, 0] > 0, 1.0, slope))
    xp = _padded(x)
    gzp = np.zeros((N, H + 2, W + 2))
    gzp[:, 1:H + 1, 1:W + 1] = gz
    gw = np.zeros((1, C, 3, 3))
    gx = np.zeros((N, C, H, W))
    for ky in range(3):
        for kx in range(3):
            for c in range(C):
                gw[0, c, ky, kx] = wscale * np.sum(gz * xp[:, c, ky:ky + H, kx:kx + W])
                # gz[n, u - ky + 1, v - kx + 1] = gzp[n, u - ky + 2, v - kx + 2]
                gx[:, c] += wscale * w[0, c, ky, kx] * gzp[:, 2 - ky:2 - ky + H, 2 - kx:2 - kx + W]
    return gx, gw, np.array([gz.sum()])


def case(shape, seed=None):
    """x, w ~ N(0, 1), b = 0.1, g ~ N(0, 1) as fp32 torch tensors on the CPU, and wscale = 1 / sqrt(9 C)."""
    import torch
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(sum(shape) if seed is None else seed)
    x = torch.randn(N, C, H, W, generator=gen)
    w = torch.randn(1, C, 3, 3, generator=gen)
    g = torch.randn(N, 1, H, W, generator=gen)
    return x, w, torch.full((1,), 0.1), g, 1.0 / (9 * C) ** 0.5
