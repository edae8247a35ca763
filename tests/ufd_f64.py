"""upfirdn2d in fp64, written from the operator's definition (a plain module: no fixtures, no pytest hooks):

    1. zero-stuff    sample i of an axis goes to position i * up of an axis of length in * up
    2. pad / crop    pad0 zeros in front and pad1 behind; a negative pad crops instead
    3. filter        correlate with the flipped taps (a true convolution), 'valid' extent
    4. decimate      keep every down-th sample, starting with the first

with up, down per axis, four pads and kh != kw.  Nothing here is taken from the kernels' index arithmetic (no mid / floor_div /
tap-phase expressions): the tests hold the kernels, the C oracle and the committed goldens to it.  Differentiable torch, so the
adjoints come from autograd.  x is [N, C, H, W]; up = (up_x, up_y), down = (down_x, down_y), pad = (x0, x1, y0, y1) in the
argument order of the C ABI.
"""
import torch
import torch.nn.functional as F


def out_size(n, up, down, pad0, pad1, k):
    return (n * up + pad0 + pad1 - k) // down + 1


def upfirdn2d_f64(x, taps, up=(1, 1), down=(1, 1), pad=(0, 0, 0, 0)):
    x, taps = x.double(), taps.double()
    n, c, h, w = x.shape
    (ux, uy), (dx, dy), (px0, px1, py0, py1) = up, down, pad
    kh, kw = taps.shape
    z = x.new_zeros((n, c, h * uy, w * ux))
    z[:, :, ::uy, ::ux] = x
    z = F.pad(z, (max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)))
    z = z[:, :, max(-py0, 0):z.shape[2] - max(-py1, 0), max(-px0, 0):z.shape[3] - max(-px1, 0)]
    fh, fw = z.shape[2] - kh + 1, z.shape[3] - kw + 1
    assert fh > 0 and fw > 0, 'empty output'
    flipped = torch.flip(taps, [0, 1])
    full = x.new_zeros((n, c, fh, fw))
    for i in range(kh):
        for j in range(kw):
            full = full + flipped[i, j] * z[:, :, i:i + fh, j:j + fw]
    return full[:, :, ::dy, ::dx]


def tail_f64(v, bias=None, noise=None, noise_w=None, act=True, slope=0.2, gain=2.0 ** 0.5):
    """gain * lrelu(v + bias[c] + noise_w * noise[n or 0]) (act = False: no activation, no gain).  v [N, C, H, W], noise [1 or N, H, W]."""
    v = v.double()
    if bias is not None:
        v = v + bias.double().view(1, -1, 1, 1)
    if noise is not None:
        v = v + float(noise_w) * noise.double().view(noise.shape[0], 1, v.shape[2], v.shape[3])
    if act:
        v = torch.where(v > 0, v, v * slope) * gain
    return v


def adjoint_f64(v, ref, slope, gain):
    """v * (ref > 0 ? 1 : slope) * gain: the activation adjoint on the activation's saved output (+0.0 and -0.0 take the slope)."""
    return v.double() * torch.where(ref.double() > 0, 1.0, float(slope)) * gain


def tile_sums_f64(v, toh, tow):
    """Per-tile channel sums of v [N, C, H, W] -> [N, tiles_y * tiles_x (row-major), C]; edge tiles hold what is in range."""
    n, c, h, w = v.shape
    ty, tx = -(-h // toh), -(-w // tow)
    p = F.pad(v.double(), (0, tx * tow - w, 0, ty * toh - h))
    return p.view(n, c, ty, toh, tx, tow).sum(dim=(3, 5)).permute(0, 2, 3, 1).reshape(n, ty * tx, c)
