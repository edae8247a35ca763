"""Independent fp64 restatement of LPIPS (lpips 0.1, VGG16 backbone), written from the definitions: scaling layer, torchvision
vgg16 features[0:30] tapped after indices 3, 8, 15, 22, 29, channel normalisation, weighted squared difference, spatial mean,
sum over taps.  Plus synthetic weights in the lpips state_dict layout and smooth test images."""
import torch
import torch.nn.functional as F

CONVS = [(0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256), (17, 256, 512),
         (19, 512, 512), (21, 512, 512), (24, 512, 512), (26, 512, 512), (28, 512, 512)]
POOL_AT = (4, 9, 16, 23)
TAP_AT = (3, 8, 15, 22, 29)
TAP_C = (64, 128, 256, 512, 512)


def _slice(idx):
    return 1 + sum(idx > b for b in TAP_AT[:4])


def synthetic_state_dict(seed, mixed_sign=False):
    """lpips.LPIPS(net='vgg').state_dict() layout: He-normal convolutions (std sqrt(2 / fan_in)) and small biases, so
    activations stay O(1) through 13 ReLU layers; lin weights U(0, 0.1), or U(-0.05, 0.1) with ``mixed_sign``."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, ci, co in CONVS:
        sd[f'net.slice{_slice(idx)}.{idx}.weight'] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd[f'net.slice{_slice(idx)}.{idx}.bias'] = torch.randn(co, generator=g) * 0.02
    for k, c in enumerate(TAP_C):
        w = torch.rand(1, c, 1, 1, generator=g) * 0.1
        if mixed_sign:
            w = w * 1.5 - 0.05
        sd[f'lin{k}.model.1.weight'] = w
        sd[f'lins.{k}.model.1.weight'] = w.clone()
    sd['scaling_layer.shift'] = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
    sd['scaling_layer.scale'] = torch.tensor([.458, .448, .450]).view(1, 3, 1, 1)
    return sd


def smooth_images(n, size, seed, low=8):
    """[n, 3, size, size] fp32 in [-1, 1]: bilinear upsampling of low x low uniform noise."""
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(n, 3, low, low, generator=g) * 2 - 1
    return F.interpolate(z, (size, size), mode='bilinear', align_corners=False).clamp(-1, 1).contiguous()


def taps_f64(sd, x):
    """x [N, 3, H, W] (already in [-1, 1], any dtype) -> the five relu taps in fp64, NCHW."""
    shift = torch.tensor([-.030, -.088, -.188], dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], dtype=torch.float64).view(1, 3, 1, 1)
    h = (x.double() - shift) / scale
    weights = {idx: (sd[f'net.slice{_slice(idx)}.{idx}.weight'].double(), sd[f'net.slice{_slice(idx)}.{idx}.bias'].double())
               for idx, _, _ in CONVS}
    taps = []
    for i in range(30):
        if i in weights:
            h = F.conv2d(h, weights[i][0], weights[i][1], 1, 1)
        elif i in POOL_AT:
            h = F.max_pool2d(h, 2, 2)
        else:
            h = torch.relu(h)
        if i in TAP_AT:
            taps.append(h)
    return taps


def normalize(f):
    return f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)


def lins_f64(sd):
    return [sd[f'lin{k}.model.1.weight'].double().flatten() for k in range(5)]


def lpips_from_taps(ta, tb, lins):
    """Paired LPIPS of two tap lists [N, C, h, w] -> [N] fp64."""
    out = 0
    for a, b, w in zip(ta, tb, lins):
        out = out + ((normalize(a) - normalize(b)) ** 2 * w.view(1, -1, 1, 1)).sum(1).mean((1, 2))
    return out


def lpips_f64(sd, x, y):
    return lpips_from_taps(taps_f64(sd, x), taps_f64(sd, y), lins_f64(sd))


def lpips_matrix_f64(sd, xa, xb):
    """[na, nb] fp64 LPIPS of every pair."""
    ta, lins = taps_f64(sd, xa), lins_f64(sd)
    tb = ta if xb is xa else taps_f64(sd, xb)
    na, nb = xa.shape[0], xb.shape[0]
    out = torch.zeros(na, nb, dtype=torch.float64)
    for i in range(na):
        out[i] = lpips_from_taps([t[i:i + 1].expand(nb, *t.shape[1:]) for t in ta], tb, lins)
    return out


def to_unit(q):
    """uint8 images -> (q / 255 - 0.5) / 0.5 in fp64 (the reference's ToTensor + Normalize)."""
    return (q.double() / 255 - 0.5) / 0.5
