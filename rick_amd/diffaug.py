"""Differentiable Augmentation (Zhao et al., NeurIPS 2020): policy ``color,translation,cutout`` applied to reals and fakes in the
D and G steps — the other standard low-data recipe next to ADA (rick_amd/augment.py).

Per image the published operator draws b ~ U(-0.5, 0.5), s ~ U(0, 2), c ~ U(0.5, 1.5), integer shifts (tr, tc) and a cutout centre,
and applies brightness, saturation, contrast, a zero-filled integer translation and a zeroed rectangle.  The three colour steps
collapse to one affine map, so the whole operator is

    y = Cut . Shift . (L x + b),      L x = (c s) x + c (1 - s) mean_ch(x) + (1 - c) mean_all(x)

with a self-adjoint L (DESIGN.md "DiffAugment").  The draws are made on the host with torch's CPU generator in the published call
order (a seed reproduces the published composition's numbers) and go to the device as a parameter block of N ``rick_diffaug_param``
records; CUDA float32 images then take two fused HIP launches per direction (rick_amd/csrc/diffaug.hip) through ``DiffAugFn`` /
``DiffAugAdjFn``, each the other's backward.  CPU tensors and other dtypes take a composed torch path on the same records.
"""
import numpy as np
import torch

from .param_block import ParamStaging, fused_launch, linear_pair, upload_params  # noqa: F401  (ParamStaging: exported here too)

__all__ = ['POLICIES', 'PARAM_DTYPE', 'parse_policy', 'shift_range', 'cut_size', 'cut_bounds', 'draw_params', 'identity_params',
           'check_params', 'apply_params', 'DiffAugFn', 'DiffAugAdjFn', 'diffaug_fused', 'diffaug']

POLICIES = ('color', 'translation', 'cutout')

# rick_diffaug_param (include/rick_hip.h)
PARAM_DTYPE = np.dtype([('b', '<f4'), ('s', '<f4'), ('c', '<f4'), ('tr', '<i4'), ('tc', '<i4'), ('r0', '<i4'), ('r1', '<i4'),
                        ('c0', '<i4'), ('c1', '<i4'), ('pad', '<i4')])
assert PARAM_DTYPE.itemsize == 40


def parse_policy(policy):
    """'color,translation,cutout' or any non-empty subset of it in that order -> tuple of stage names; ValueError otherwise."""
    if not isinstance(policy, str) or not policy:
        raise ValueError(f'diffaug: the policy must be a non-empty string of {",".join(POLICIES)}; got {policy!r}')
    parts = tuple(policy.split(','))
    if any(p not in POLICIES for p in parts) or len(set(parts)) != len(parts) or list(parts) != sorted(parts, key=POLICIES.index):
        raise ValueError(f'diffaug: the policy must be a subset of {",".join(POLICIES)} in that order; got {policy!r}')
    return parts


def shift_range(size):
    """Largest translation of a dimension: int(size * 0.125 + 0.5)."""
    return int(size * 0.125 + 0.5)


def cut_size(size):
    """Cutout extent of a dimension: int(size * 0.5 + 0.5)."""
    return int(size * 0.5 + 0.5)


def identity_params(n):
    """N records of the identity: b = 0, s = 1, c = 1, no shift, an empty cut."""
    out = np.zeros(n, PARAM_DTYPE)
    out['s'] = 1.0
    out['c'] = 1.0
    return out


def cut_bounds(centre, size):
    """The rows clamp(centre - CH // 2 + i, 0, size - 1), i < CH, as a half-open range: never empty, always inside."""
    ch = cut_size(size)
    lo = np.clip(centre - ch // 2, 0, size - 1)
    hi = np.clip(centre - ch // 2 + ch - 1, 0, size - 1) + 1
    return lo, hi


def draw_params(n, h, w, policy, generator=None):
    """The draws of one call on n images of h x w as PARAM_DTYPE records, made on the CPU with torch's generator in the published
    order and shapes: brightness rand(n,1,1,1), saturation, contrast, then randint [n,1,1] for the row shift, the column shift, the
    cut row and the cut column; the stages the policy leaves out draw nothing."""
    stages = parse_policy(policy) if isinstance(policy, str) else tuple(policy)
    out = identity_params(n)
    kw = dict(generator=generator)
    if 'color' in stages:
        out['b'] = (torch.rand(n, 1, 1, 1, **kw) - 0.5).view(n).numpy()
        out['s'] = (torch.rand(n, 1, 1, 1, **kw) * 2).view(n).numpy()
        out['c'] = (torch.rand(n, 1, 1, 1, **kw) + 0.5).view(n).numpy()
    if 'translation' in stages:
        sr, sc = shift_range(h), shift_range(w)
        out['tr'] = torch.randint(-sr, sr + 1, size=[n, 1, 1], **kw).view(n).numpy()
        out['tc'] = torch.randint(-sc, sc + 1, size=[n, 1, 1], **kw).view(n).numpy()
    if 'cutout' in stages:
        orow = torch.randint(0, h + (1 - cut_size(h) % 2), size=[n, 1, 1], **kw).view(n).numpy()
        ocol = torch.randint(0, w + (1 - cut_size(w) % 2), size=[n, 1, 1], **kw).view(n).numpy()
        out['r0'], out['r1'] = cut_bounds(orow, h)
        out['c0'], out['c1'] = cut_bounds(ocol, w)
    return out


def check_params(params, h, w):
    """ValueError for records the kernels' contract excludes: |tr| >= h, |tc| >= w, cut bounds outside the image, NaN (host side:
    the device block cannot be inspected without a synchronisation)."""
    from ._lib import lib
    params = np.ascontiguousarray(params, dtype=PARAM_DTYPE)
    if params.size < 1 or lib.rick_diffaug_check_params(params.ctypes.data, int(params.size), int(h), int(w)) != 0:
        raise ValueError(f'diffaug: parameter records do not fit a {h}x{w} image')
    return params


# ------------------------------------------------------------------------------------------ composed torch path (any device / dtype)
def apply_params(img, params):
    """The operator for given records as a composition of torch ops in img's dtype (differentiable; the CPU path of diffaug())."""
    n, ch, h, w = img.shape
    if ch != 3 or len(params) != n:
        raise ValueError(f'diffaug: needs [N, 3, H, W] images and N records; got {tuple(img.shape)}, {len(params)}')

    def col(name):
        return torch.as_tensor(np.asarray(params[name], dtype=np.float64), device=img.device).to(img.dtype).view(n, 1, 1, 1)

    x = img + col('b')
    m = x.mean(dim=1, keepdim=True)
    x = (x - m) * col('s') + m
    m = x.mean(dim=[1, 2, 3], keepdim=True)
    x = (x - m) * col('c') + m
    rows = torch.arange(h, device=img.device).view(1, h, 1)
    cols = torch.arange(w, device=img.device).view(1, 1, w)

    def icol(name):
        return torch.as_tensor(np.asarray(params[name], dtype=np.int64), device=img.device).view(n, 1, 1)

    sr, sc = rows + icol('tr'), cols + icol('tc')
    live = (sr >= 0) & (sr < h) & (sc >= 0) & (sc < w)
    live = live & ~((rows >= icol('r0')) & (rows < icol('r1')) & (cols >= icol('c0')) & (cols < icol('c1')))
    batch = torch.arange(n, device=img.device).view(n, 1, 1)
    moved = x.permute(0, 2, 3, 1)[batch, sr.clamp(0, h - 1), sc.clamp(0, w - 1)].permute(0, 3, 1, 2)
    return moved * live.unsqueeze(1).to(img.dtype)


# ------------------------------------------------------------------------------------------------------- fused path (HIP, host side)
def _workspace(lib, n, h, w, device):
    nbytes = int(lib.rick_diffaug_workspace_bytes(n, h, w))
    if nbytes < 0:
        raise RuntimeError(f'diffaug: unsupported image shape {(n, 3, h, w)}')
    return torch.empty(nbytes // 8, device=device, dtype=torch.float64)


# y = diffaug(x) for fixed per-image draws (`bias`: with the brightness offset) and the adjoint of its linear part, each the other's
# backward; no gradient flows to the parameters.
DiffAugFn, DiffAugAdjFn = linear_pair(fused_launch('diffaug', PARAM_DTYPE.itemsize, 'rick_diffaug', _workspace),
                                      'DiffAugFn', 'DiffAugAdjFn')


def diffaug_fused(img, params):
    """DiffAugment of CUDA float32 [N, 3, H, W] images with a device parameter block of N rick_diffaug_param entries."""
    return DiffAugFn.apply(img, params, True)


def diffaug(img, policy, generator=None):
    """Draw (CPU generator, published order) and apply: the fused HIP path for CUDA float32 images, the composed torch path for
    everything else."""
    n, _, h, w = img.shape
    params = draw_params(n, h, w, policy, generator)
    if img.is_cuda and img.dtype == torch.float32:
        return diffaug_fused(img, upload_params(check_params(params, h, w), img.device))
    return apply_params(img, params)
