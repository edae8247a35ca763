"""fp64 expressions of the small kernels that run between the layers on every training step (rick_amd/csrc/elementwise.hip: the
ResBlock merge, masked Adam, EMA, the Fisher accumulation and per-filter means, minibatch stddev; rick_amd/csrc/split.hip: running
maxima and the bound of an activation tail; rick_amd/csrc/data.hip: the image batch) and the byte-level host model of a split image,
written out from include/rick_hip.h for tests/test_gpu_state_forms.py.  The value functions take fp32 CPU tensors and
fp32-representable Python floats and return fp64.  A plain module: no fixtures, no device."""
import numpy as np
import torch

U = 2.0 ** -24
AMAX_SLOTS, AMAX_STRIDE, AMAX_FLOATS = 16, 32, 512
SPLIT_TARGET = 13             # a split image's bound is placed in [2^13, 2^14)
MBSTD_EPS = float(np.float32(1e-8))


# ------------------------------------------------------------------------------------------------------ split images
def f32_bits(v):
    return int(np.float32(v).view(np.uint32))


def bits_f32(b):
    return np.uint32(b).view(np.float32)


def pow2_scale(bound, T=SPLIT_TARGET):
    """The exponent rule in integer arithmetic: bound (fp32, >= 0, finite) -> (2^e, 2^-e, clamp) with bound * 2^e in [2^T, 2^(T+1))
    unless a clamp acted: 'zero' (bound 0: e = 0), 'low' (biased exponent below T + 1: e = 126), 'high' (above 253: e = T - 126)."""
    bits = f32_bits(bound)
    assert bits >> 31 == 0
    eb, clamp = (bits >> 23) & 0xFF, None
    if bits == 0:
        eb, clamp = 127 + T, 'zero'
    elif eb < T + 1:
        eb, clamp = T + 1, 'low'
    elif eb > 253:
        eb, clamp = 253, 'high'
    return bits_f32((254 + T - eb) << 23), bits_f32((eb - T) << 23), clamp


def amax_read(word):
    """The value of an amax word: the maximum over its 16 slots (fp32)."""
    return np.float32(np.asarray(word, dtype=np.float32)[::AMAX_STRIDE].max())


def split_header(word0, word1, coef):
    """{2^e, 2^-e, bound, 0} with bound = coef * (amax0 [+ amax1]) in fp32 as written -> (4 x fp32, clamp)."""
    tot = amax_read(word0) + (amax_read(word1) if word1 is not None else np.float32(0))
    bound = np.float32(coef) * np.float32(tot)
    scale, unscale, clamp = pow2_scale(bound)
    return np.array([scale, unscale, bound, 0], dtype=np.float32), clamp


def split_image(x, scale):
    """The documented format, byte for byte: the 16 bytes of every four values hold {hi x 4 | lo x 4}, hi = fp16(v 2^e),
    lo = fp16(v 2^e - hi), both to nearest even (v 2^e and the difference are exact in fp32).  x: fp32, numel % 4 == 0 -> uint8."""
    w = np.asarray(x, dtype=np.float32).reshape(-1, 4) * np.float32(scale)
    hi = w.astype(np.float16)
    lo = (w - hi.astype(np.float32)).astype(np.float16)
    ht = torch.from_numpy(w).half()
    lt = (torch.from_numpy(w) - ht.float()).half()
    assert np.array_equal(ht.numpy().view(np.uint16), hi.view(np.uint16)) and np.array_equal(lt.numpy().view(np.uint16), lo.view(np.uint16)), \
        'numpy and torch disagree about an fp16 conversion'
    return np.ascontiguousarray(np.concatenate([hi, lo], axis=1)).view(np.uint8).reshape(-1)


def split_halves_of(img):
    """uint8 image -> (hi, lo) as fp16 arrays [n / 4, 4]."""
    h = np.asarray(img, dtype=np.uint8).view(np.float16).reshape(-1, 8)
    return h[:, :4], h[:, 4:]


def split_decode(img, unscale):
    """(hi + lo) * 2^-e in fp32, as rick_split_unpack_f32 writes it."""
    hi, lo = split_halves_of(img)
    return ((hi.astype(np.float32) + lo.astype(np.float32)) * np.float32(unscale)).reshape(-1)


# ------------------------------------------------------------------------------------------------------- elementwise
def add_scale(a, b, alpha):
    """y = (a + b) * alpha -> (y, sum |terms|)"""
    return (a.double() + b.double()) * alpha, (a.double().abs() + b.double().abs()) * abs(alpha)


def bound_tail(a_w0, c0, nw, a_noise, bias, gain, mul):
    """max |mul| * gain * (c0 * amax(w0) + max |nw| * amax(w_noise) + max |bias|); absent terms dropped, absent factor 1."""
    v = c0 * float(a_w0) + (float(bias.double().abs().max()) if bias is not None else 0.0)
    if nw is not None and a_noise is not None:
        v += abs(float(nw)) * float(a_noise)
    return (float(mul.double().abs().max()) if mul is not None else 1.0) * gain * v


def masked_adam_moments(p, g, m, v, mask, beta1, beta2):
    """Prune p, zero g, then torch.optim.Adam's moments in its lerp form:
    m' = m + (g - m)(1 - beta1), v' = v beta2 + (1 - beta2) g^2 -> (p pruned, g masked, m', sum |terms|, v', sum |terms|)"""
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    if mask is not None:
        p = torch.where((mask & 2) != 0, torch.zeros_like(p), p)
        g = torch.where((mask & 3) != 0, torch.zeros_like(g), g)
    om1, om2 = 1.0 - beta1, 1.0 - beta2
    mn, Sm = m + (g - m) * om1, m.abs() + (g.abs() + m.abs()) * om1
    vn = v * beta2 + om2 * g * g
    return p, g, mn, Sm, vn, vn.clone()


def adam_update(p, m, v, lr, eps, bc1, bc2):
    """p' = p - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps) from the NEW moments -> (p', |update|)"""
    t = (lr / bc1) * (m.double() / (v.double().sqrt() / bc2 ** 0.5 + eps))
    return p.double() - t, t.abs()


def ema(e, p, decay):
    a, b = e.double() * decay, p.double() * (1.0 - decay)
    return a + b, a.abs() + b.abs()


def sq_accumulate(acc, g):
    return acc.double() + g.double() ** 2


def filter_reduce(X, scale):
    """X [outer, nfilters, inner] -> out[f] = scale * sum_{o,i} X[o,f,i], and scale * sum |X|"""
    return scale * X.double().sum((0, 2)), scale * X.double().abs().sum((0, 2))


# ------------------------------------------------------------------------------------------------- minibatch stddev
def mbstd_compose(x, gout, groups, dtype):
    """The formula of include/rick_hip.h in `dtype` by plain tensor composition: x [B, P, C], gout [B, P, C + 1] (or None) ->
    (stat [groups], gx [B, P, C] or None).  fp64: the reference; fp32: the composition the project's 4x rule measures against."""
    B, P, C = x.shape
    gs, PC = B // groups, P * C
    xg = x.to(dtype).reshape(groups, gs, PC)
    mean = xg.sum(1, keepdim=True) / gs
    d = xg - mean
    var = (d * d).sum(1, keepdim=True)
    sd = (var / gs + torch.tensor(MBSTD_EPS, dtype=dtype)).sqrt()
    stat = sd.sum(2).reshape(groups) / PC
    if gout is None:
        return stat, None
    gg = gout.to(dtype).reshape(groups, gs, P, C + 1)
    G = gg[..., C].sum((1, 2)) / PC
    gx = gg[..., :C].reshape(groups, gs, PC) + G[:, None, None] * d / (gs * sd)
    return stat, gx.reshape(B, P, C)


def mbstd_stat_bound(x, groups):
    """A-priori bound on |device stat - fp64 stat| per run, every step of mbstd_fwd_kernel counted (1 ulp = 2 U for a division
    and for sqrtf):
      mean   gs - 1 additions on partial sums of at most A = sum_b |x_b| and one division: e_mean <= (gs + 1) U A / gs
      d_b    = x_b - mean, one rounding: |d_b' - d_b| <= delta_b = e_mean (1 + U) + U |d_b|
      var    sum_b d_b'^2: 2 |d_b| delta_b + delta_b^2 per term, then gs products and gs additions on positive terms:
             (gs + 1) U relative (the first addition, to 0, is exact)
      arg    var / gs + 1e-8f: a division (2 U on var / gs) and an addition (U on arg)
      sd     sqrt is monotone and sqrt(a') - sqrt(a) = (a' - a) / (sqrt(a') + sqrt(a)); sqrtf adds 2 U sd
      stat   positive terms: ceil(PC / 1024) thread-local additions, 6 wave-shuffle levels, 16 in the block's fixed-order sum,
             then the division by PC (2 U), plus one ulp of the result; 1 % on top for the second-order terms."""
    B, P, C = x.shape
    gs, PC = B // groups, P * C
    xg = x.double().reshape(groups, gs, PC)
    d = xg - xg.mean(1, keepdim=True)
    var = (d * d).sum(1)
    arg = var / gs + MBSTD_EPS
    sd = arg.sqrt()
    stat = sd.sum(1) / PC
    A = xg.abs().sum(1)
    e_mean = (gs + 1) * U * A / gs
    delta = e_mean[:, None, :] * (1 + U) + U * d.abs()
    var_err = (2 * d.abs() * delta + delta * delta).sum(1)
    var_err = var_err + (gs + 1) * U * (var + var_err)
    arg_err = var_err / gs + 2 * U * var / gs + U * arg
    sd_err = arg_err / (sd + (arg - arg_err).clamp_min(0).sqrt()) + 2 * U * sd
    T = -(-PC // 1024)
    err = (sd_err.sum(1) + (T + 6 + 16) * U * sd.sum(1)) / PC + 2 * U * stat
    _, e = torch.frexp(stat.float())
    return 1.01 * err + 2.0 ** (e.double() - 24)


# ------------------------------------------------------------------------------------------------------ image batch
def image_table():
    """The 256 values (u8 / 255 - 0.5) / 0.5 takes, evaluated in fp32 on the CPU (ToTensor, then Normalize(0.5, 0.5))."""
    v = np.arange(256, dtype=np.float32) / np.float32(255.0)
    return (v - np.float32(0.5)) / np.float32(0.5)


def image_batch(images, index, flip, table):
    """images uint8 [N, H, W, 3], index, flip [B] -> [B, 3, H, W] fp32 (numpy)."""
    out = []
    for i, f in zip(index, flip):
        im = images[int(i)]
        out.append(np.transpose(table[im[:, ::-1] if f else im], (2, 0, 1)))
    return np.stack(out)
