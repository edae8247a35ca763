"""Oracle of the ADA image path (helper, not collected): rick_aug_param semantics as include/rick_hip.h and the head comment of
rick_amd/csrc/augment.hip state them, in fp64, from ONE parameter-block entry and a [3, H, W] image.  Nothing of
random_apply_affine, upfirdn2d or grid_sample: index gathers and two plain convolutions, so fp64 autograd of <out, gy> is the
exact transpose.

    padded[u, v] = x[refl(u - py1 - 6, H), refl(v - px1 - 6, W)]                       on the hp x wp canvas
    up[Y, X]     = sum_{a,b} z[Y + a, X + b] k2[a][b],  z the zero-stuffed 2x canvas   (2hp - 11) x (2wp - 11)
    region[r, c] = bilinear sample of `up` at ix = a0 c + a1 r + a2, iy = a3 c + a4 r + a5, r < 2H + 10, c < 2W + 10;
                   a corner outside the canvas contributes 0
    d[i, j]      = sum_{a,b} region[2i + a, 2j + b] k2[11 - a][11 - b]
    out          = col[:, :3] d (+ col[:, 3])

k2 is torch.outer of the fp32 sym6 taps taken to fp64: the values the kernels multiply by.  ix, iy are evaluated as the kernels
evaluate them (two fp64 fused multiply-adds each, emulated exactly with rationals), so the floor decisions are the kernels'.

``mode`` selects what runs through the pipeline:
    'value'   the definition;
    'tight'   |x| with |k2|, |col| and the (non-negative) bilinear weights: S_tight, the sum of the absolute terms;
    'corner'  the same with every in-canvas corner weight replaced by 1: S_corner;
    'count'   indicator inputs (x != 0, col != 0, k2 -> 1, in-canvas corner -> 1): the number of paths that reach an element.
``adjoint`` transposes whichever mode by autograd.  ``adj_chain`` is the length of aug_warp_adj_kernel's accumulation chain per
source pixel; ``apply_f32`` / ``adjoint_f32`` evaluate the definition in fp32 in the kernels' order (tap by tap, vectorised over
pixels; one source pixel at a time for the warp adjoint) and serve only to measure the CPU bases of the sharp check."""
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

SYM6 = (0.015404109327027373, 0.0034907120842174702, -0.11799011114819057, -0.048311742585633,
        0.4910559419267466, 0.787641141030194, 0.3379294217276218, -0.07263752278646252,
        -0.021060292512300564, 0.04472490177066578, 0.0017677118642428036, -0.007800708325034148)
KT, PADK = 12, 6


def k2_f32():
    taps = torch.tensor(SYM6, dtype=torch.float32)
    return torch.outer(taps, taps)


def refl(t, n):
    t = np.abs(t)
    return np.where(t > n - 1, 2 * (n - 1) - t, t)


def pads_of(prm, H, W):
    """(px1, px2, py1, py2) of an entry."""
    px1, py1 = int(prm['px1']), int(prm['py1'])
    return px1, int(prm['wp']) - W - px1 - 2 * PADK, py1, int(prm['hp']) - H - py1 - 2 * PADK


def _fma(a, b, c):
    """fma(a, b, c) of doubles, one rounding."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def structure(prm, H, W):
    """The integer side of one entry: reflect index vectors, canvas sizes and, per region pixel, the floor corner, the
    fractions (fp64, exact) and which of the 4 corners lie inside the canvas."""
    px1, px2, py1, py2 = pads_of(prm, H, W)
    hp, wp = int(prm['hp']), int(prm['wp'])
    assert min(px1, px2, py1, py2) >= 0 and max(px1, px2) + PADK < W and max(py1, py2) + PADK < H
    a = [float(v) for v in prm['a']]
    RH, RW = 2 * H + 10, 2 * W + 10
    ix, iy = np.empty((RH, RW)), np.empty((RH, RW))
    for r in range(RH):
        bx, by = _fma(a[1], float(r), a[2]), _fma(a[4], float(r), a[5])
        for c in range(RW):
            ix[r, c], iy[r, c] = _fma(a[0], float(c), bx), _fma(a[3], float(c), by)
    x0, y0 = np.floor(ix), np.floor(iy)
    s = dict(H=H, W=W, hp=hp, wp=wp, H2=2 * hp - 11, W2=2 * wp - 11, RH=RH, RW=RW, pads=(px1, px2, py1, py2),
             ri=refl(np.arange(hp) - py1 - PADK, H), ci=refl(np.arange(wp) - px1 - PADK, W),
             x0=x0.astype(np.int64), y0=y0.astype(np.int64), fx=ix - x0, fy=iy - y0, det=a[0] * a[4] - a[1] * a[3], a=a)
    assert s['ri'].min() >= 0 and s['ri'].max() < H and s['ci'].min() >= 0 and s['ci'].max() < W
    return s


def corners(s):
    """[(flat canvas index, weight fp64, inside) per corner], in the kernels' order (dy outer, dx inner)."""
    out = []
    for dy in (0, 1):
        Y = s['y0'] + dy
        wy = s['fy'] if dy else 1.0 - s['fy']
        for dx in (0, 1):
            X = s['x0'] + dx
            wx = s['fx'] if dx else 1.0 - s['fx']
            inside = (Y >= 0) & (Y < s['H2']) & (X >= 0) & (X < s['W2'])
            idx = np.where(inside, Y * s['W2'] + X, 0)
            out.append((torch.from_numpy(idx.reshape(-1)), torch.from_numpy(wy * wx), torch.from_numpy(inside)))
    return out


def from_padded(padded, s, col, bias, mode):
    """padded [C, hp, wp] fp64 (C a multiple of 3: images stacked along the channels) -> out [C, H, W]."""
    k2 = k2_f32().double()
    k2 = {'value': k2, 'tight': k2.abs(), 'corner': k2.abs(), 'count': torch.ones_like(k2)}[mode]
    C = padded.shape[0]
    z = torch.zeros(C, 2 * s['hp'], 2 * s['wp'], dtype=torch.float64)
    z[:, ::2, ::2] = padded
    up = F.conv2d(z[:, None], k2[None, None])[:, 0].reshape(C, -1)
    region = 0
    for idx, wt, inside in corners(s):
        wgt = torch.where(inside, wt if mode in ('value', 'tight') else torch.ones_like(wt), torch.zeros_like(wt))
        region = region + up[:, idx].reshape(C, s['RH'], s['RW']) * wgt
    d = F.conv2d(region[:, None], torch.flip(k2, (0, 1))[None, None], stride=2)[:, 0]
    m = torch.as_tensor(np.asarray(col, dtype=np.float64).reshape(3, 4))
    m = {'value': m, 'tight': m.abs(), 'corner': m.abs(), 'count': (m != 0).double()}[mode]
    out = torch.einsum('ij,bjhw->bihw', m[:, :3], d.view(-1, 3, s['H'], s['W']))
    return (out + m[:, 3].view(3, 1, 1) if bias else out).reshape(C, s['H'], s['W'])


def _input(x, mode):
    x = x.double()
    return {'value': x, 'tight': x.abs(), 'corner': x.abs(), 'count': (x != 0).double()}[mode]


def _linear(x, prm, bias, mode, s):
    """x [3, H, W] or [B, 3, H, W] (B images under the one entry)."""
    s = s or structure(prm, x.shape[-2], x.shape[-1])
    flat = x.reshape(-1, s['H'], s['W'])
    padded = flat[:, torch.from_numpy(s['ri'])][:, :, torch.from_numpy(s['ci'])]
    return from_padded(padded, s, prm['col'], bias, mode).reshape(x.shape)


def apply(x, prm, bias=True, mode='value', s=None):
    return _linear(_input(x, mode), prm, bias, mode, s)


def adjoint(gy, prm, mode='value', s=None):
    """The transpose of the linear part (of whichever mode) applied to gy [3, H, W]."""
    x = torch.zeros(gy.shape, dtype=torch.float64, requires_grad=True)
    return torch.autograd.grad((_linear(x, prm, False, mode, s) * _input(gy, mode)).sum(), x)[0]


def padded_weight(prm, H, W, s=None):
    """[hp, wp]: sum over outputs of the absolute weight with which a padded-canvas pixel reaches them ('corner' mode, identity
    colour): which reflect copies matter."""
    s = s or structure(prm, H, W)
    padded = torch.ones(3, s['hp'], s['wp'], dtype=torch.float64, requires_grad=True)
    out = from_padded(padded, s, np.eye(3, 4).reshape(-1), False, 'corner')
    return torch.autograd.grad(out.sum(), padded)[0][0]


def _copy_counts(lo_rows, hi_rows, index, n):
    """[P, n]: how many canvas positions u in [lo_rows[P], hi_rows[P]] reflect to source index s."""
    m = np.zeros((lo_rows.size, n))
    for u, sidx in enumerate(index):
        m[:, sidx] += (lo_rows <= u) & (u <= hi_rows)
    return m


def adj_chain(prm, H, W, s=None):
    """[H, W]: the number of (reflect copy, region pixel) pairs aug_warp_adj_kernel adds for a source pixel: the pairs with at
    least one bilinear corner inside the copy's 12 x 12 tap box clipped to the canvas.  Rows and columns decide independently:
    copy u serves canvas rows [2u - 11, 2u], so an in-canvas corner row Y is served by u in [ceil(Y / 2), floor((Y + 11) / 2)]."""
    s = s or structure(prm, H, W)

    def span(f0, size):
        f0 = f0.reshape(-1)
        lo, hi = np.maximum(f0, 0), np.minimum(f0 + 1, size - 1)                # the in-canvas corner rows, empty if lo > hi
        return np.where(lo <= hi, -(-lo // 2), 1), np.where(lo <= hi, (hi + 11) // 2, 0)
    mu = _copy_counts(*span(s['y0'], s['H2']), s['ri'], H)
    mv = _copy_counts(*span(s['x0'], s['W2']), s['ci'], W)
    return torch.from_numpy(mu.T @ mv)


def features(prm, H, W, s=None):
    """The edge geometries an entry reaches, from the block and the structure above alone."""
    s = s or structure(prm, H, W)
    px1, px2, py1, py2 = s['pads']
    a = s['a']
    f = set()
    if min(s['pads']) == 0:
        f.add('pad0')
    if px1 != px2 and py1 != py2:
        f.add('pad-asym')
    if px1 != py1 and H != W:
        f.add('pad-xy-differ')
    if (max(px1, px2) > 0 and max(px1, px2) + PADK == W - 1) or (max(py1, py2) > 0 and max(py1, py2) + PADK == H - 1):
        f.add('pad-limit')
    if H == 7 and W == 7:
        f.add('min-image')
    if H == 7 and W > 7:
        f.add('min-image-7xW')
    if any(not bool(inside.all()) for _, _, inside in corners(s)):
        f.add('oob-corner')
    if (s['fx'] == 0).any() or (s['fy'] == 0).any():
        f.add('int-coords')
    if s['det'] < 0:
        f.add('flip')
    axis, cross = max(abs(a[0]), abs(a[4])), max(abs(a[1]), abs(a[3]))
    if axis < 1e-6 and cross > 0.5 and H != W:
        f.add('rot90-nonsquare')
    if min(abs(a[0]), abs(a[1]), abs(a[3]), abs(a[4])) > 0.1 and min(s['pads']) > 0:
        f.add('rotation')
    if cross < 1e-6 and abs(abs(a[0]) - abs(a[4])) > 0.05:
        f.add('aniso')
    # reflect copies that carry weight: canvas rows / columns below the image (mirrored low) or above it (mirrored high); the
    # outermost canvas row / column is the copy of s == lo + 6 resp. s == n - 1 - (hi + 6), the last source pixel that has one
    wgt = padded_weight(prm, H, W, s)
    rows, cols = wgt.sum(1) > 0, wgt.sum(0) > 0
    if bool(rows[:py1 + PADK].any()) or bool(cols[:px1 + PADK].any()):
        f.add('mirror-lo')
    if bool(rows[py1 + PADK + H:].any()) or bool(cols[px1 + PADK + W:].any()):
        f.add('mirror-hi')
    if bool(rows[0]) or bool(cols[0]):
        f.add('mirror-lo-edge')
    if bool(rows[-1]) or bool(cols[-1]):
        f.add('mirror-hi-edge')
    return f


# ------------------------------------------------------------------------------------------------- fp32, the kernels' order
def _weights_f32(s):
    fx, fy = s['fx'].astype(np.float32), s['fy'].astype(np.float32)
    one = np.float32(1)
    return fx, fy, one - fx, one - fy


def apply_f32(x, prm, bias=True):
    """aug_warp_fwd_kernel + aug_down_fwd_kernel in numpy fp32: the same taps in the same order, a multiply and an add where the
    kernels fuse them."""
    x = x.numpy().astype(np.float32)
    H, W = x.shape[1:]
    s = structure(prm, H, W)
    px1, _, py1, _ = s['pads']
    k2 = k2_f32().numpy()
    fx, fy, gx, gy = _weights_f32(s)
    region = np.zeros((3, s['RH'], s['RW']), np.float32)
    for dy in (0, 1):
        Y = s['y0'] + dy
        for dx in (0, 1):
            X = s['x0'] + dx
            inside = (Y >= 0) & (Y < s['H2']) & (X >= 0) & (X < s['W2'])
            wt = (fy if dy else gy) * (fx if dx else gx)
            a0, b0 = Y & 1, X & 1
            v = np.zeros_like(region)
            for i in range(6):
                sy = refl((Y + a0 + 2 * i) // 2 - py1 - PADK, H).clip(0, H - 1)
                for j in range(6):
                    sx = refl((X + b0 + 2 * j) // 2 - px1 - PADK, W).clip(0, W - 1)
                    v = v + x[:, sy, sx] * k2[a0 + 2 * i, b0 + 2 * j]
            region = np.where(inside, region + wt * v, region)
    d = np.zeros((3, H, W), np.float32)
    for a in range(KT):
        for b in range(KT):
            d = d + region[:, a:a + 2 * H:2, b:b + 2 * W:2] * k2[KT - 1 - a, KT - 1 - b]
    m = np.asarray(prm['col'], np.float32).reshape(3, 4)
    out = np.empty_like(d)
    for ch in range(3):
        v = np.full((H, W), m[ch, 3] if bias else 0, np.float32)
        for k in range(3):
            v = v + m[ch, k] * d[k]
        out[ch] = v
    return torch.from_numpy(out)


def adjoint_f32(gy, prm, fault=None):
    """aug_down_adj_kernel + aug_warp_adj_kernel in numpy fp32, in the kernels' order.  `fault` plants one of the index faults the
    device checks must notice (the tests of the tests): 'edge-copy' drops the outermost reflect copy (canvas row 0, the copy of
    s == lo + 6), 'short-box' the last region pixel of every tap box, 'colour' transposes the colour matrix."""
    g = gy.numpy().astype(np.float32)
    H, W = g.shape[1:]
    s = structure(prm, H, W)
    RH, RW = s['RH'], s['RW']
    k2 = k2_f32().numpy()
    gp = np.zeros((3, H + 11, W + 11), np.float32)                              # row i of gy at 5 + i + 1: zero where i is outside
    gp[:, 6:6 + H, 6:6 + W] = g
    r, c = np.meshgrid(np.arange(RH), np.arange(RW), indexing='ij')
    acc = np.zeros((3, RH, RW), np.float32)
    for di in range(6):                                                         # ascending i: i = (r - 10) // 2 + di (floor), a = r - 2i
        ii = (r - KT + 2) // 2 + di
        a = r - 2 * ii
        for dj in range(6):
            jj = (c - KT + 2) // 2 + dj
            b = c - 2 * jj
            ok = (a >= 0) & (a < KT) & (b >= 0) & (b < KT)
            t = np.where(ok, k2[(KT - 1 - a).clip(0, 11), (KT - 1 - b).clip(0, 11)], np.float32(0))
            acc = acc + gp[:, (ii + 6).clip(0, H + 10), (jj + 6).clip(0, W + 10)] * t
    m = np.asarray(prm['col'], np.float32).reshape(3, 4)
    gw = np.empty_like(acc)
    for ch in range(3):
        col = m[ch, :3] if fault == 'colour' else m[:3, ch]
        v = col[0] * acc[0]
        v = v + col[1] * acc[1]
        gw[ch] = v + col[2] * acc[2]
    gw = gw.reshape(3, -1)
    fx, fy, gx1, gy1 = _weights_f32(s)
    out = np.zeros((3, H, W), np.float32)
    us = [[u for u in (sy + s['pads'][2] + PADK, -sy + s['pads'][2] + PADK, 2 * (H - 1) - sy + s['pads'][2] + PADK)
           if 0 <= u < s['hp'] and s['ri'][u] == sy] for sy in range(H)]
    vs = [[v for v in (sx + s['pads'][0] + PADK, -sx + s['pads'][0] + PADK, 2 * (W - 1) - sx + s['pads'][0] + PADK)
           if 0 <= v < s['wp'] and s['ci'][v] == sx] for sx in range(W)]
    for sy in range(H):
        for sx in range(W):
            tot = np.zeros(3, np.float32)
            for u in dict.fromkeys(us[sy]):
                if fault == 'edge-copy' and u == 0:
                    continue
                Ylo, Yhi = max(0, 2 * u - 11), min(s['H2'] - 1, 2 * u)
                for v in dict.fromkeys(vs[sx]):
                    Xlo, Xhi = max(0, 2 * v - 11), min(s['W2'] - 1, 2 * v)
                    wsum = np.zeros((RH, RW), np.float32)
                    hit = np.zeros((RH, RW), bool)
                    for dy in (0, 1):
                        Y = s['y0'] + dy
                        for dx in (0, 1):
                            X = s['x0'] + dx
                            ok = (Y >= Ylo) & (Y <= Yhi) & (X >= Xlo) & (X <= Xhi)
                            wt = (fy if dy else gy1) * (fx if dx else gx1)
                            t = k2[(2 * u - Y).clip(0, 11), (2 * v - X).clip(0, 11)]
                            wsum = np.where(ok, wsum + wt * t, wsum)
                            hit |= ok
                    sel = np.flatnonzero(hit.reshape(-1))[:-1 if fault == 'short-box' else None]
                    ws = wsum.reshape(-1)
                    for k in sel:
                        tot = tot + ws[k] * gw[:, k]
            out[:, sy, sx] = tot
    return torch.from_numpy(out)
