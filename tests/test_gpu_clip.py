"""GPU: the CLIP image-tower kernels (rick_amd/csrc/clip.hip and the linear epilogue of the f32 implicit GEMM) through the C
ABI against fp64 references, the whole network against the independent fp64 restatement (tests/clip_f64.py) and against
the golden embeddings of an implementation the author did not write, batch invariance, graph capture, and the evaluator's
FID / KID in CLIP space end to end.  The conftest's autouse fixture asserts after every test that the saturation counter stayed
at 0.

Tolerances: the rule of tests/test_gpu_vgg.py.  For every comparison the base figure is the error of the fp32 torch CPU
composition against the same fp64 reference on the same inputs (max error over the reference's max-norm, measured once on
the CPU and written down below next to its shape); the device bound is that figure x 4."""
import math
import os

import numpy as np
import pytest
import torch

from tests.clip_f64 import (SmoothG, affine_f64, bicubic_f64, clip_images, embed_f64, max_rel_err, synthetic_clip_state_dict)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0
FACTOR = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clip_tiny.npz')

# fp32 torch CPU (F.interpolate bicubic + the affine) against the fp64 rule on input_images(h, w), resized to 224
INPUT_CPU_BASE = {(256, 256): 3.568e-05, (64, 64): 8.942e-06, (299, 299): 4.806e-05, (100, 317): 3.463e-05}
# fp32 torch CPU act(F.linear(x, w, b)) [+ res] against fp64 on gemm_inputs(name), keyed name -> {(act, with res): base}
GEMM_SHAPES = {'51x64x192': (51, 64, 192), '51x72x64': (51, 72, 64), '150x768x3072': (150, 768, 3072), '129x256x64': (129, 256, 64),
               'patch': None}                                    # K = 72: no multiple of 32; M = 129: one row past a 128-row tile
GEMM_CPU_BASE = {'51x64x192': {(0, False): 2.211e-07, (0, True): 1.438e-07, (1, False): 3.181e-07, (1, True): 1.793e-07},
                 '51x72x64': {(0, False): 2.916e-07, (0, True): 1.794e-07, (1, False): 3.283e-07, (1, True): 2.089e-07},
                 '150x768x3072': {(0, False): 6.461e-07, (0, True): 4.484e-07, (1, False): 7.547e-07, (1, True): 4.927e-07},
                 '129x256x64': {(0, False): 5.218e-07, (0, True): 3.590e-07, (1, False): 5.471e-07, (1, True): 4.002e-07},
                 'patch': {(0, False): 1.450e-06, (0, True): 8.748e-07, (1, False): 1.295e-06, (1, True): 7.378e-07}}
# fp32 torch CPU F.layer_norm against fp64 on layernorm_inputs(R, C)
LN_CPU_BASE = {(51, 64): 1.070e-07, (51, 768): 1.351e-07, (3, 1024): 7.693e-08, (5, 36): 8.110e-08}
LN_STRIDED_CPU_BASE = 7.415e-08                                  # every 17th row of 3 x 17 rows of 64
LN_OFFSET_CPU_BASE = 2.829e-06                                   # 51 x 768, mean 100, standard deviation 1
# fp32 torch CPU softmax(q k^T / sqrt(d)) v against fp64 on attention_inputs(T, d, heads): (as is, queries x 30)
ATT_CPU_BASE = {(17, 16, 4): (2.544e-07, 2.679e-06), (50, 64, 2): (4.312e-07, 6.144e-06), (82, 32, 2): (5.882e-07, 6.030e-06),
                (257, 64, 1): (1.254e-06, 1.186e-05)}
# fp32 torch CPU network (ClipImageFeatures on CPU tensors) against the fp64 restatement on network_inputs(cfg, size)[:n]
NET_CPU_BASE = {('A', 32, 3): 5.115e-07, ('A', 32, 27): 4.612e-07, ('A', 64, 3): 4.940e-07, ('A', 64, 27): 5.119e-07,
                ('B', 256, 3): 2.191e-06, ('B', 256, 27): 1.832e-06}
GOLDEN_CPU_BASE = 2.510e-07                                      # the golden's weights and images against the golden's embeddings

CONFIGS = {'A': (dict(width=64, patch=8, image=32, layers=2, mlp=256, dim=32), 4),      # (cfg, heads): d = 16, T = 17
           'B': (dict(width=128, patch=8, image=56, layers=1, mlp=512, dim=64), 2)}     # d = 64, T = 50


def _lib():
    from rick_amd import _lib
    return _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def quickgelu_f64(u):
    return u / (1 + torch.exp(-1.702 * u))


# ---- input kernel ---------------------------------------------------------------------------------------------------------
def input_images(h, w):
    return torch.rand(2, 3, h, w, generator=_gen(1000 * h + w)) * 2 - 1


def run_input(x, size):
    L = _lib()
    n, _, h, w = x.shape
    xd = x.to(DEV)
    out = torch.full((n + 1, size, size, 4), SENTINEL, device=DEV)              # one guard image behind the output
    L.check(L.lib.rick_clip_input_f32(xd.data_ptr(), out.data_ptr(), n, h, w, size, L.stream_ptr()), 'rick_clip_input_f32')
    assert torch.all(out[n] == SENTINEL)
    return out[:n].cpu()


def test_input_kernel_copies_at_the_output_size():
    x = input_images(32, 32)
    mean, std = (torch.tensor(v).view(1, 3, 1, 1) for v in ((0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)))
    got = run_input(x, 32)
    assert torch.equal(got[..., :3], ((x * 0.5 + 0.5 - mean) / std).permute(0, 2, 3, 1))    # the affine alone, bit for bit
    assert torch.all(got[..., 3] == 0)


@pytest.mark.parametrize('hw', list(INPUT_CPU_BASE))
def test_input_kernel_vs_fp64_bicubic(hw):
    x = input_images(*hw)
    ref = affine_f64(bicubic_f64(x, 224)).permute(0, 2, 3, 1)
    got = run_input(x, 224)
    err, base = max_rel_err(got[..., :3], ref), INPUT_CPU_BASE[hw]
    print(f'rick_clip_input_f32 {hw} -> 224: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.all(got[..., 3] == 0)
    assert torch.equal(run_input(x, 224), got)


# ---- GEMM epilogue --------------------------------------------------------------------------------------------------------
_GEMM_CACHE = {}


def gemm_inputs(name):
    """x, the layer (w [N, K] as a convolution filter, b [N]) and a residual [M, N]; 'patch' is the patch-embedding geometry:
    3 images of 64 x 64 x 4 (channel 3 = 0) under a 32 x 32 stride-32 filter onto 64 columns, K = 4096, M = 12."""
    if name not in _GEMM_CACHE:
        g = _gen(sum(map(ord, name)))
        if name == 'patch':
            x = torch.randn(3, 64, 64, 4, generator=g)
            x[..., 3] = 0
            w, geom = torch.randn(64, 3, 32, 32, generator=g) * 3072 ** -0.5, (3, 64, 64, 4, (32, 32), (32, 32))
            M, N = 12, 64
        else:
            M, K, N = GEMM_SHAPES[name]
            x = torch.randn(M, K, generator=g)
            w, geom = torch.randn(N, K, 1, 1, generator=g) * K ** -0.5, (M, 1, 1, K, (1, 1), (1, 1))
        _GEMM_CACHE[name] = (x, w, torch.randn(N, generator=g) * 0.1, torch.randn(M, N, generator=g), geom)
    return _GEMM_CACHE[name]


def gemm_reference(name, act, with_res, dtype=torch.float64):
    """act(conv(x) + b) [+ res] as [M, N], in `dtype` on the CPU."""
    x, w, b, res, geom = gemm_inputs(name)
    if name == 'patch':
        y = torch.nn.functional.conv2d(x.to(dtype).permute(0, 3, 1, 2)[:, :3], w.to(dtype), b.to(dtype), stride=geom[5])
        y = y.permute(0, 2, 3, 1).reshape(res.shape)
    else:
        y = torch.nn.functional.linear(x.to(dtype), w.to(dtype)[:, :, 0, 0], b.to(dtype))
    if act:
        y = y * torch.sigmoid(1.702 * y) if dtype == torch.float32 else quickgelu_f64(y)
    return y + res.to(dtype) if with_res else y


class _Gemm:
    """One packed layer on the device and its launch on the first `rows` GEMM rows (images)."""

    def __init__(self, name):
        from rick_amd import gemm_conv
        self.x, w, b, self.res, self.geom = gemm_inputs(name)
        self.n_cols = w.shape[0]
        wpk, bias, self.cop, self.bn = gemm_conv.pack(w, b, ci_pad=4 if name == 'patch' else None)
        self.wpk, self.bias, self.xd = wpk.to(DEV), bias.to(DEV), self.x.to(DEV)
        self.rows_per_image = self.res.shape[0] // self.x.shape[0]

    def __call__(self, act, res, images=None, xd=None):
        """res: None, 'separate' or 'inplace'."""
        from rick_amd import gemm_conv
        L = _lib()
        n, h, w, ci, k, s = self.geom
        n = images or n
        m = n * self.rows_per_image
        xd = self.xd if xd is None else xd
        out = torch.full((m + 1, self.n_cols), SENTINEL, device=DEV)           # one guard row behind the output
        rd = None
        if res == 'separate':
            rd = self.res[:m].to(DEV)
        elif res == 'inplace':
            out[:m] = self.res[:m].to(DEV)
            rd = out
        a = gemm_conv.descriptor(n, h, w, ci, k, s, (0, 0), self.cop, self.bn, [(out.data_ptr(), self.n_cols, 0, self.n_cols)])
        L.check(L.lib.rick_inc_conv_lin_f32(xd.data_ptr(), self.wpk.data_ptr(), self.bias.data_ptr(), None if rd is None else rd.data_ptr(),
                                            int(act), a, L.stream_ptr()), 'rick_inc_conv_lin_f32')
        assert torch.all(out[m] == SENTINEL)
        return out[:m]


@pytest.mark.parametrize('name', list(GEMM_SHAPES))
def test_gemm_epilogue_vs_fp64(name):
    gemm = _Gemm(name)
    for act in (0, 1):
        for res in (None, 'separate', 'inplace'):
            ref = gemm_reference(name, act, res is not None)
            got = gemm(act, res)
            err, base = max_rel_err(got.cpu(), ref), GEMM_CPU_BASE[name][(act, res is not None)]
            print(f'rick_inc_conv_lin_f32 {name} act={act} res={res}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, '
                  f'bound {FACTOR * base:.3e})')
            assert err <= FACTOR * base
            assert torch.equal(gemm(act, res), got)                          # run to run
            if res == 'inplace':
                assert torch.equal(got, gemm(act, 'separate'))               # the same sums, the same bits


def test_gemm_rows_do_not_depend_on_the_other_rows():
    gemm = _Gemm('129x256x64')
    full = gemm(1, 'separate')
    assert torch.equal(gemm(1, 'separate', images=128), full[:128])          # one tile instead of two
    assert torch.equal(gemm(1, 'separate', images=1), full[:1])
    other = torch.randn(129, 256, generator=_gen(3)).to(DEV)
    other[5] = gemm.xd[5]
    assert torch.equal(gemm(1, 'separate', xd=other)[5], full[5])            # row 5 beside different rows


def test_gemm_epilogue_rejects_what_it_does_not_support():
    from rick_amd import gemm_conv
    L = _lib()
    t = torch.zeros(1 << 14, device=DEV)
    p = t.data_ptr()
    ok = lambda: gemm_conv.descriptor(4, 1, 1, 64, (1, 1), (1, 1), (0, 0), 64, 64, [(p, 64, 0, 64)])      # noqa: E731
    assert L.lib.rick_inc_conv_lin_f32(p, p, p, None, 0, ok(), L.stream_ptr()) == 0
    assert L.lib.rick_inc_conv_lin_f32(p, p, p, None, 2, ok(), L.stream_ptr()) == 22                      # unknown activation
    assert L.lib.rick_inc_conv_lin_f32(p, p, None, None, 0, ok(), L.stream_ptr()) == 22
    two = gemm_conv.descriptor(4, 1, 1, 64, (1, 1), (1, 1), (0, 0), 64, 64, [(p, 64, 0, 32), (p, 64, 32, 32)])
    assert L.lib.rick_inc_conv_lin_f32(p, p, p, None, 0, two, L.stream_ptr()) == 22                       # one destination only
    odd = gemm_conv.descriptor(4, 1, 1, 62, (1, 1), (1, 1), (0, 0), 64, 64, [(p, 64, 0, 64)])
    assert L.lib.rick_inc_conv_lin_f32(p, p, p, None, 0, odd, L.stream_ptr()) == 22                       # K % 4
    torch.cuda.synchronize()


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------
def layernorm_inputs(R, C):
    g = _gen(R * 10000 + C)
    return torch.randn(R, C, generator=g) * 1.5 + 0.3, 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


def layernorm_f64(x, w, b):
    x = x.double()
    mu = x.mean(1, keepdim=True)
    return (x - mu) / torch.sqrt(((x - mu) ** 2).mean(1, keepdim=True) + 1e-5) * w.double() + b.double()


def run_layernorm(x, w, b, rows=None, ldx=None):
    """x: a flat or [R, C] buffer; rows / ldx: R rows read with the row stride ldx."""
    L = _lib()
    C = w.numel()
    R = rows if rows is not None else x.shape[0]
    xd, wd, bd = x.to(DEV).contiguous(), w.to(DEV), b.to(DEV)
    out = torch.full((R + 1, C), SENTINEL, device=DEV)
    L.check(L.lib.rick_clip_layernorm_f32(xd.data_ptr(), ldx or C, wd.data_ptr(), bd.data_ptr(), out.data_ptr(), R, C, 1e-5,
                                          L.stream_ptr()), 'rick_clip_layernorm_f32')
    assert torch.all(out[R] == SENTINEL)
    return out[:R].cpu()


@pytest.mark.parametrize('R,C', list(LN_CPU_BASE))
def test_layernorm_vs_fp64(R, C):
    x, w, b = layernorm_inputs(R, C)
    got = run_layernorm(x, w, b)
    err, base = max_rel_err(got, layernorm_f64(x, w, b)), LN_CPU_BASE[(R, C)]
    print(f'rick_clip_layernorm_f32 {R} x {C}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.equal(run_layernorm(x, w, b), got)


def test_layernorm_reads_rows_with_a_stride():
    x, w, b = layernorm_inputs(51, 64)                        # 3 images of 17 tokens: token 0 of every image
    got = run_layernorm(x, w, b, rows=3, ldx=17 * 64)
    err = max_rel_err(got, layernorm_f64(x[::17], w, b))
    print(f'rick_clip_layernorm_f32 every 17th row: {err:.3e} (fp32 CPU {LN_STRIDED_CPU_BASE:.3e}, bound {FACTOR * LN_STRIDED_CPU_BASE:.3e})')
    assert err <= FACTOR * LN_STRIDED_CPU_BASE
    assert torch.equal(got, run_layernorm(x[::17].contiguous(), w, b))


def test_layernorm_of_constant_rows_is_the_bias():
    """The constants and C copies of them add up exactly in fp32 (small integers times powers of two), so the mean is the
    constant, every deviation is 0 and the result is the bias, bit for bit."""
    for C in (36, 64, 768, 1024):
        _, w, b = layernorm_inputs(5, C)
        x = torch.tensor([3.0, -0.5, 100.0, 0.0, 0.015625])[:, None].expand(5, C).contiguous()
        assert torch.equal(run_layernorm(x, w, b), b.expand(5, C))


def test_layernorm_with_a_large_mean():
    """Rows with mean 100 and standard deviation 1: E[x^2] - mean^2 in fp32 loses what the two passes keep."""
    x, w, b = layernorm_inputs(51, 768)
    x = (x - 0.3) / 1.5 + 100
    got = run_layernorm(x, w, b)
    err = max_rel_err(got, layernorm_f64(x, w, b))
    print(f'rick_clip_layernorm_f32 mean 100, std 1: {err:.3e} (fp32 CPU {LN_OFFSET_CPU_BASE:.3e}, bound {FACTOR * LN_OFFSET_CPU_BASE:.3e})')
    assert err <= FACTOR * LN_OFFSET_CPU_BASE


def test_layernorm_and_tokens_reject_what_they_do_not_support():
    L = _lib()
    t = torch.zeros(1 << 14, device=DEV)
    p, s = t.data_ptr(), L.stream_ptr()
    assert L.lib.rick_clip_layernorm_f32(p, 64, p, p, p, 4, 64, 1e-5, s) == 0
    for R, C, ldx in ((4, 62, 64), (4, 2052, 2052), (4, 64, 32), (4, 64, 66), (-1, 64, 64)):
        assert L.lib.rick_clip_layernorm_f32(p, ldx, p, p, p, R, C, 1e-5, s) == 22
    assert L.lib.rick_clip_layernorm_f32(None, 64, p, p, p, 4, 64, 1e-5, s) == 22
    assert L.lib.rick_clip_tokens_f32(p, p, p, p, p, p, 2, 258, 16, 1e-5, s) == 22
    assert L.lib.rick_clip_tokens_f32(p, p, p, p, p, p, 2, 5, 18, 1e-5, s) == 22
    torch.cuda.synchronize()


def test_tokens_kernel_vs_fp64():
    """[class ; patches] + positional embedding, then ln_pre: against fp64 with LayerNorm's 51 x 64 base, and bit for bit
    against the LayerNorm kernel on the sums formed on the host (one fp32 addition per element either way)."""
    L = _lib()
    N, T, C = 3, 17, 64
    g = _gen(77)
    patches, cls, pos = torch.randn(N, T - 1, C, generator=g), torch.randn(C, generator=g), torch.randn(T, C, generator=g)
    _, w, b = layernorm_inputs(51, 64)
    out = torch.full((N * T + 1, C), SENTINEL, device=DEV)
    dev = [v.to(DEV) for v in (patches, cls, pos, w, b)]
    L.check(L.lib.rick_clip_tokens_f32(*(v.data_ptr() for v in dev), out.data_ptr(), N, T, C, 1e-5, L.stream_ptr()), 'rick_clip_tokens_f32')
    assert torch.all(out[N * T] == SENTINEL)
    rows = (torch.cat([cls.expand(N, 1, C), patches], 1) + pos).reshape(N * T, C)
    got = out[:N * T].cpu()
    err = max_rel_err(got, layernorm_f64(rows, w, b))
    print(f'rick_clip_tokens_f32 3 x 17 x 64: {err:.3e} (fp32 CPU LayerNorm 51 x 64 {LN_CPU_BASE[(51, 64)]:.3e})')
    assert err <= FACTOR * LN_CPU_BASE[(51, 64)]
    assert torch.equal(got, run_layernorm(rows, w, b))


# ---- attention ------------------------------------------------------------------------------------------------------------
def attention_inputs(T, d, heads, qscale=1.0):
    qkv = torch.randn(3, T, 3, heads * d, generator=_gen(T * 100 + d))
    qkv[:, :, 0] *= qscale
    return qkv.reshape(3, T, 3 * heads * d).contiguous()


def attention_reference(qkv, d, heads, dtype=torch.float64):
    n, T, _ = qkv.shape
    q, k, v = (u.reshape(n, T, heads, d).transpose(1, 2) for u in qkv.to(dtype).reshape(n, T, 3, heads * d).unbind(2))
    return (torch.softmax(q @ k.transpose(2, 3) / math.sqrt(d), -1) @ v).transpose(1, 2).reshape(n, T, heads * d)


def run_attention(qkv, d, heads):
    L = _lib()
    n, T, _ = qkv.shape
    qd = qkv.to(DEV).contiguous()
    out = torch.full((n * T + 1, heads * d), SENTINEL, device=DEV)
    L.check(L.lib.rick_clip_attention_f32(qd.data_ptr(), out.data_ptr(), n, T, heads, d, L.stream_ptr()), 'rick_clip_attention_f32')
    assert torch.all(out[n * T] == SENTINEL)
    return out[:n * T].view(n, T, heads * d).cpu()


@pytest.mark.parametrize('T,d,heads', list(ATT_CPU_BASE))
def test_attention_vs_fp64(T, d, heads):
    for i, qscale in enumerate((1.0, 30.0)):                  # x 30: scores of several hundred, the max subtraction at work
        qkv = attention_inputs(T, d, heads, qscale)
        got = run_attention(qkv, d, heads)
        err, base = max_rel_err(got, attention_reference(qkv, d, heads)), ATT_CPU_BASE[(T, d, heads)][i]
        print(f'rick_clip_attention_f32 T={T} d={d} heads={heads} q x {qscale:g}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, '
              f'bound {FACTOR * base:.3e})')
        assert torch.isfinite(got).all()
        assert err <= FACTOR * base
        assert torch.equal(run_attention(qkv, d, heads), got)


@pytest.mark.parametrize('T,d,heads', [(17, 16, 4), (257, 64, 1)])
def test_attention_of_an_image_does_not_depend_on_the_batch(T, d, heads):
    qkv = attention_inputs(T, d, heads)
    full = run_attention(qkv, d, heads)
    assert torch.equal(run_attention(qkv[1:2], d, heads), full[1:2])          # alone
    assert torch.equal(run_attention(qkv.flip(0), d, heads)[2], full[0])      # last in a batch
    other = torch.randn(qkv.shape, generator=_gen(9))
    other[1] = qkv[1]
    assert torch.equal(run_attention(other, d, heads)[1], full[1])            # beside different images


def test_attention_rejects_what_it_does_not_support():
    L = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    p, s = t.data_ptr(), L.stream_ptr()
    assert L.lib.rick_clip_attention_f32(p, p, 1, 5, 2, 16, s) == 0
    for T, heads, d in ((258, 1, 16), (0, 1, 16), (5, 2, 48), (5, 2, 128), (5, 0, 16)):
        assert L.lib.rick_clip_attention_f32(p, p, 1, T, heads, d, s) == 22
    assert L.lib.rick_clip_attention_f32(None, p, 1, 5, 2, 16, s) == 22
    torch.cuda.synchronize()


# ---- whole network --------------------------------------------------------------------------------------------------------
_NETS, _NET_REF = {}, {}


def network(name, layout='transformers'):
    from rick_amd.clip import ClipImageFeatures
    if (name, layout) not in _NETS:
        cfg, heads = CONFIGS[name]
        _NETS[(name, layout)] = ClipImageFeatures.load(synthetic_clip_state_dict(cfg, 11, layout), device=DEV, batch=25, heads=heads)
    return _NETS[(name, layout)]


def network_inputs(name, size):
    return clip_images(27, size, seed=size + ord(name))


def network_reference(name, size):
    if (name, size) not in _NET_REF:
        cfg, heads = CONFIGS[name]
        _NET_REF[(name, size)] = embed_f64(synthetic_clip_state_dict(cfg, 11), network_inputs(name, size), heads)
    return _NET_REF[(name, size)]


@pytest.mark.parametrize('name,size,n', list(NET_CPU_BASE))
def test_network_vs_fp64(name, size, n):
    net = network(name)
    x = network_inputs(name, size)[:n].to(DEV)
    got = net(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, CONFIGS[name][0]['dim']) and got.device.type == 'cuda'
    err, base = max_rel_err(got.cpu(), network_reference(name, size)[:n]), NET_CPU_BASE[(name, size, n)]
    print(f'CLIP {name} from {size}^2, n={n}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.equal(net(x), got)                                           # run to run


def test_network_on_the_golden_weights_vs_the_golden_embeddings():
    from rick_amd.clip import ClipImageFeatures
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    net = ClipImageFeatures.load(sd, device=DEV, heads=2)
    got = net(torch.from_numpy(z['images']).to(DEV))
    err = max_rel_err(got.cpu(), torch.from_numpy(z['image_embeds']))
    print(f'CLIP golden: max err / max-norm {err:.3e} (fp32 CPU {GOLDEN_CPU_BASE:.3e}, bound {FACTOR * GOLDEN_CPU_BASE:.3e})')
    assert err <= FACTOR * GOLDEN_CPU_BASE


@pytest.mark.parametrize('name,size', [('A', 64), ('B', 256)])
def test_both_layouts_give_the_same_bits(name, size):
    x = network_inputs(name, size)[:5].to(DEV)
    want = network(name)(x)
    for layout in ('openai', 'openai-visual'):
        assert torch.equal(network(name, layout)(x), want)


@pytest.mark.parametrize('name,size', [('A', 64), ('B', 256)])
def test_embeddings_do_not_depend_on_the_batch(name, size):
    net = network(name)
    x = network_inputs(name, size).to(DEV)
    full = net(x)                                             # chunks of 25 + 2
    assert torch.equal(net(x[:3]), full[:3])
    assert torch.equal(net(x[24:27]), full[24:27])            # image 24: last of a chunk there, first of one here
    assert torch.equal(net(x[26:27]), full[26:27])
    assert torch.equal(net(x.flip(0)).flip(0), full)


def test_graph_capture_replays_the_eager_result():
    net = network('A')
    x = network_inputs('A', 64)
    eager = net(x[:5].to(DEV))
    static = x[:5].to(DEV).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        net(static)                                           # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = net(static)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    static.copy_(x[5:10])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, net(x[5:10].to(DEV)))


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_evaluator_fid_and_kid_in_clip_space():
    from rick_amd.evaluate import Evaluator, clip_similarity
    net = network('A')
    g = SmoothG(32).to(DEV)
    real = clip_images(48, 32, seed=5).to(DEV)
    seen = []

    def feature_fn(img):
        f = net(img)
        seen.append(f)
        return f
    ev = Evaluator(g, feature_fn, net(real), n_sample_store=16, inception_nsamples=48, fid_sample_size=48)
    z = torch.randn(48, 512, generator=_gen(39))
    score = ev.compute_inception_score(fid=True, kid=True, latents=z, kid_subsets=4, kid_subset_size=24, rng=np.random.RandomState(0))
    assert all(f.device.type == 'cuda' and f.dtype == torch.float32 and tuple(f.shape) == (16, 32) for f in seen)
    print(f"CLIP-space FID {float(score['fid']):.4f}, KID {float(score['kid']):.5f}")
    assert math.isfinite(float(score['fid'])) and float(score['fid']) > 0
    assert math.isfinite(float(score['kid']))
    sim = clip_similarity(seen[0], net(real))
    assert sim.device.type == 'cuda' and sim.dtype == torch.float64 and tuple(sim.shape) == (16, 48)
    assert float(sim.abs().max()) <= 1 + 1e-12
