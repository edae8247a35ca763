"""Oracles of DiffAugment (helper, not collected).

``compose``  the seven published steps one by one (brightness, saturation, contrast, translation by a padded gather, cutout by a
             scattered mask), written from the operator's definition, in the dtype of x, drawing from torch's global CPU RNG in the
             published order (the draws themselves are fp32, as ``torch.rand`` makes them, and are then cast).
``apply``    the closed form  y = Cut . Shift . (L x + b)  in fp64 for given parameter records, ``linear`` its linear part and
             ``adjoint`` the transpose of that — slicing only, differentiable by autograd."""
import numpy as np
import torch
import torch.nn.functional as F


def shift_range(size):
    return int(size * 0.125 + 0.5)


def cut_size(size):
    return int(size * 0.5 + 0.5)


# ------------------------------------------------------------------------------------------------------------- the published steps
def compose(x, policy):
    n, _, h, w = x.shape
    for stage in policy.split(','):
        if stage == 'color':
            x = x + (torch.rand(n, 1, 1, 1) - 0.5).to(x.dtype)
            mean = x.mean(dim=1, keepdim=True)
            x = (x - mean) * (torch.rand(n, 1, 1, 1) * 2).to(x.dtype) + mean
            mean = x.mean(dim=[1, 2, 3], keepdim=True)
            x = (x - mean) * (torch.rand(n, 1, 1, 1) + 0.5).to(x.dtype) + mean
        elif stage == 'translation':
            sr, sc = shift_range(h), shift_range(w)
            tr = torch.randint(-sr, sr + 1, size=[n, 1, 1])
            tc = torch.randint(-sc, sc + 1, size=[n, 1, 1])
            gb, gr, gc = torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), indexing='ij')
            gr = torch.clamp(gr + tr + 1, 0, h + 1)
            gc = torch.clamp(gc + tc + 1, 0, w + 1)
            padded = F.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
            x = padded.permute(0, 2, 3, 1).contiguous()[gb, gr, gc].permute(0, 3, 1, 2)
        elif stage == 'cutout':
            ch, cw = cut_size(h), cut_size(w)
            orow = torch.randint(0, h + (1 - ch % 2), size=[n, 1, 1])
            ocol = torch.randint(0, w + (1 - cw % 2), size=[n, 1, 1])
            gb, gr, gc = torch.meshgrid(torch.arange(n), torch.arange(ch), torch.arange(cw), indexing='ij')
            gr = torch.clamp(gr + orow - ch // 2, min=0, max=h - 1)
            gc = torch.clamp(gc + ocol - cw // 2, min=0, max=w - 1)
            mask = torch.ones(n, h, w, dtype=x.dtype)
            mask[gb, gr, gc] = 0
            x = x * mask.unsqueeze(1)
        else:
            raise ValueError(stage)
    return x


# ------------------------------------------------------------------------------------------------------------------ the closed form
def _col(params, name, n):
    return torch.from_numpy(np.asarray(params[name], dtype=np.float64).reshape(n)).view(n, 1, 1, 1)


def linear(x, params):
    """L x = (c s) x + c (1 - s) mean_ch(x) + (1 - c) mean_all(x), fp64."""
    x = x.double()
    n = x.shape[0]
    c, s = _col(params, 'c', n), _col(params, 's', n)
    return c * s * x + c * (1 - s) * x.mean(dim=1, keepdim=True) + (1 - c) * x.mean(dim=[1, 2, 3], keepdim=True)


def _window(t, size):
    """Destination rows [a, b) whose source row + t lies inside [0, size)."""
    return max(0, -t), min(size, size - t)


def select(w, params):
    """Cut . Shift: y[:, r, q] = w[:, r + tr, q + tc] inside the image and outside the cut, else 0."""
    n, _, h, wd = w.shape
    out = []
    for i in range(n):
        tr, tc = int(params['tr'][i]), int(params['tc'][i])
        (ra, rb), (qa, qb) = _window(tr, h), _window(tc, wd)
        y = torch.zeros_like(w[i])
        if ra < rb and qa < qb:
            y[:, ra:rb, qa:qb] = w[i][:, ra + tr:rb + tr, qa + tc:qb + tc]
        r0, r1, c0, c1 = (int(params[k][i]) for k in ('r0', 'r1', 'c0', 'c1'))
        if r0 < r1 and c0 < c1:
            y[:, r0:r1, c0:c1] = 0
        out.append(y)
    return torch.stack(out)


def select_t(gy, params):
    """Shift^T . Cut."""
    n, _, h, wd = gy.shape
    out = []
    for i in range(n):
        g = gy[i].clone()
        r0, r1, c0, c1 = (int(params[k][i]) for k in ('r0', 'r1', 'c0', 'c1'))
        if r0 < r1 and c0 < c1:
            g[:, r0:r1, c0:c1] = 0
        tr, tc = int(params['tr'][i]), int(params['tc'][i])
        (ra, rb), (qa, qb) = _window(tr, h), _window(tc, wd)
        gw = torch.zeros_like(g)
        if ra < rb and qa < qb:
            gw[:, ra + tr:rb + tr, qa + tc:qb + tc] = g[:, ra:rb, qa:qb]
        out.append(gw)
    return torch.stack(out)


def apply(x, params, bias=True):
    """y = Cut . Shift . (L x + b) in fp64 (`bias=False`: the linear part)."""
    w = linear(x, params)
    if bias:
        w = w + _col(params, 'b', x.shape[0])
    return select(w, params)


def adjoint(gy, params):
    """gx = L . Shift^T . Cut . gy in fp64 (L is self-adjoint)."""
    return linear(select_t(gy.double(), params), params)
