"""GPU: what DINOv2's ViT (rick_amd/dinov2.py) adds to the CLIP transformer's kernels, through the C ABI against fp64
references (the ViT epilogue of the f32 implicit GEMM, the input kernel with the constants as arguments, the stem without
ln_pre), the whole network against the independent fp64 restatement (tests/dinov2_f64.py) and against the golden outputs of
an implementation the author did not write, both layouts, batch invariance, graph capture, and the evaluator's FD / KID in
DINOv2 space end to end.  The conftest's autouse fixture asserts after every test that the saturation counter stayed at 0.

Tolerances: the rule of tests/test_gpu_clip.py.  For every comparison the base figure is the error of the fp32 torch CPU
composition against the same fp64 reference on the same inputs (max error over the reference's max-norm, measured once on
the CPU and written down below next to its shape); the device bound is that figure x 4."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.dinov2_f64 import (CLIP_MEAN, CLIP_STD, MEAN, STD, SmoothG, affine_f64, bicubic_f64, clip_images, features_f64, gelu_f64,
                              max_rel_err, synthetic_dinov2_state_dict)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0
FACTOR = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dinov2_tiny.npz')

# fp32 torch CPU act(F.linear(x, w, b)) [* scale] [+ res] against fp64 on gemm_inputs(name), keyed name -> {(act, with scale,
# with res): base}.  K = 72: no multiple of 32; M = 129: one row past a 128-row tile.
GEMM_SHAPES = {'51x64x192': (51, 64, 192), '51x72x64': (51, 72, 64), '129x256x64': (129, 256, 64)}
GEMM_CPU_BASE = {
    '51x64x192': {(0, False, False): 2.211e-07, (0, False, True): 1.438e-07, (0, True, False): 2.603e-07, (0, True, True): 1.439e-07,
                  (1, False, False): 3.536e-07, (1, False, True): 1.884e-07, (1, True, False): 3.137e-07, (1, True, True): 1.484e-07},
    '51x72x64': {(0, False, False): 2.916e-07, (0, False, True): 1.794e-07, (0, True, False): 3.458e-07, (0, True, True): 1.990e-07,
                 (1, False, False): 3.852e-07, (1, False, True): 2.399e-07, (1, True, False): 3.514e-07, (1, True, True): 2.236e-07},
    '129x256x64': {(0, False, False): 5.218e-07, (0, False, True): 3.590e-07, (0, True, False): 4.210e-07, (0, True, True): 3.194e-07,
                   (1, False, False): 5.541e-07, (1, False, True): 4.047e-07, (1, True, False): 4.949e-07, (1, True, True): 3.695e-07}}
# fp32 torch CPU (F.interpolate bicubic + ImageNet's affine) against the fp64 rule on input_images(h, w), resized to 56
INPUT_CPU_BASE = {(64, 64): 7.819e-06, (100, 317): 3.145e-05}
# fp32 torch CPU network (Dinov2Features on CPU tensors) against the fp64 restatement on network_inputs(cfg, px)[:n]
NET_CPU_BASE = {('A', 56, 3): 3.450e-07, ('A', 56, 27): 4.517e-07, ('A', 256, 3): 1.985e-06, ('A', 256, 27): 2.490e-06,
                ('B', 128, 3): 7.488e-07, ('B', 128, 27): 7.376e-07}
GOLDEN_CPU_BASE = {56: 1.195e-06, 42: 5.328e-07}                             # the golden's weights and images against the golden's outputs

CONFIGS = {'A': (dict(width=64, patch=14, image=56, layers=2, mlp=256), 4),       # (cfg, heads): d = 16, T = 17
           'B': (dict(width=128, patch=14, image=98, layers=1, mlp=512), 2)}      # d = 64, T = 50


def _lib():
    from rick_amd import _lib
    return _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the ViT epilogue of the GEMM -----------------------------------------------------------------------------------------
_GEMM_CACHE = {}


def gemm_inputs(name):
    """x [M, K], the layer (w [N, K], b [N]), a LayerScale vector [N] and a residual [M, N]."""
    if name not in _GEMM_CACHE:
        g = _gen(sum(map(ord, name)))
        M, K, N = GEMM_SHAPES[name]
        x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
        _GEMM_CACHE[name] = (x, w, torch.randn(N, generator=g) * 0.1, torch.randn(M, N, generator=g),
                             0.5 + 0.5 * torch.rand(N, generator=_gen(7 + sum(map(ord, name)))))
    return _GEMM_CACHE[name]


def gemm_reference(name, act, with_scale, with_res, dtype=torch.float64):
    """act(x w^T + b) [* scale] [+ res] as [M, N], in `dtype` on the CPU."""
    x, w, b, res, scale = gemm_inputs(name)
    y = F.linear(x.to(dtype), w.to(dtype), b.to(dtype))
    if act:
        y = F.gelu(y) if dtype == torch.float32 else gelu_f64(y)
    if with_scale:
        y = y * scale.to(dtype)
    return y + res.to(dtype) if with_res else y


class _Gemm:
    """One layer packed with the column block bn on the device and its launch on the first `rows` rows."""

    def __init__(self, name, bn, layer=None):
        from rick_amd import gemm_conv
        self.x, w, b, self.res, self.scale = layer or gemm_inputs(name)
        self.n_cols, self.k = w.shape
        wpk, bias, self.cop, self.bn = gemm_conv.pack(w[:, :, None, None], b, bn=bn)
        assert self.bn == bn
        self.wpk, self.bias, self.xd, self.sd = wpk.to(DEV), bias.to(DEV), self.x.to(DEV), self.scale.to(DEV)

    def __call__(self, act, scale, res, rows=None, xd=None):
        """scale: whether the LayerScale vector is given; res: None, 'separate' or 'inplace'."""
        from rick_amd import gemm_conv
        L = _lib()
        m = rows or self.x.shape[0]
        xd = self.xd if xd is None else xd
        out = torch.full((m + 1, self.n_cols), SENTINEL, device=DEV)           # one guard row behind the output
        rd = None
        if res == 'separate':
            rd = self.res[:m].to(DEV)
        elif res == 'inplace':
            out[:m] = self.res[:m].to(DEV)
            rd = out
        a = gemm_conv.descriptor(m, 1, 1, self.k, (1, 1), (1, 1), (0, 0), self.cop, self.bn, [(out.data_ptr(), self.n_cols, 0, self.n_cols)])
        L.check(L.lib.rick_inc_conv_vit_f32(xd.data_ptr(), self.wpk.data_ptr(), self.bias.data_ptr(), self.sd.data_ptr() if scale else None,
                                            None if rd is None else rd.data_ptr(), int(act), a, L.stream_ptr()), 'rick_inc_conv_vit_f32')
        assert torch.all(out[m] == SENTINEL)
        return out[:m]


@pytest.mark.parametrize('name', list(GEMM_SHAPES))
def test_vit_epilogue_vs_fp64(name):
    narrow, wide = _Gemm(name, 64), _Gemm(name, 128)
    for act in (0, 1):
        for scale in (False, True):
            for res in (None, 'separate', 'inplace'):
                ref = gemm_reference(name, act, scale, res is not None)
                got = narrow(act, scale, res)
                err, base = max_rel_err(got.cpu(), ref), GEMM_CPU_BASE[name][(act, scale, res is not None)]
                print(f'rick_inc_conv_vit_f32 {name} act={act} scale={scale} res={res}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, '
                      f'bound {FACTOR * base:.3e})')
                assert err <= FACTOR * base
                assert torch.equal(wide(act, scale, res), got)                # the sums do not depend on the column block
                assert torch.equal(narrow(act, scale, res), got)              # run to run
                if res == 'inplace':
                    assert torch.equal(got, narrow(act, scale, 'separate'))   # the same sums, the same bits


def test_vit_epilogue_without_gelu_and_scale_is_the_linear_epilogue():
    """act = 0 and no scale: the operations of rick_inc_conv_lin_f32's act = 0 epilogue, so its bits."""
    from rick_amd import gemm_conv
    L = _lib()
    gemm = _Gemm('129x256x64', 64)
    m = 129
    for res in (None, gemm.res.to(DEV)):
        out = torch.full((m, 64), SENTINEL, device=DEV)
        a = gemm_conv.descriptor(m, 1, 1, 256, (1, 1), (1, 1), (0, 0), gemm.cop, 64, [(out.data_ptr(), 64, 0, 64)])
        L.check(L.lib.rick_inc_conv_lin_f32(gemm.xd.data_ptr(), gemm.wpk.data_ptr(), gemm.bias.data_ptr(), None if res is None else res.data_ptr(),
                                            0, a, L.stream_ptr()), 'rick_inc_conv_lin_f32')
        assert torch.equal(gemm(0, False, None if res is None else 'separate'), out)


@pytest.mark.parametrize('bn', [64, 128])
def test_vit_epilogue_rows_do_not_depend_on_the_other_rows(bn):
    gemm = _Gemm('129x256x64', bn)
    full = gemm(1, True, 'separate')
    assert torch.equal(gemm(1, True, 'separate', rows=128), full[:128])       # one tile instead of two
    assert torch.equal(gemm(1, True, 'separate', rows=1), full[:1])
    other = torch.randn(129, 256, generator=_gen(3)).to(DEV)
    other[5] = gemm.xd[5]
    assert torch.equal(gemm(1, True, 'separate', xd=other)[5], full[5])       # row 5 beside different rows


@pytest.mark.parametrize('bn', [64, 128])
def test_gelu_epilogue_at_the_ends_of_its_range(bn):
    """Row r of x is (u_r, 0, 0, 0) and every filter is (1, 0, 0, 0) with a zero bias: the accumulator, and so the activation's
    argument, is u_r.  erff is exactly +-1 from |u| = 6 on: +40 comes back as 40, -40 as a zero.  Against the fp64 GELU over the
    largest value: the expression is four roundings of 2^-24 (three products and a sum) and an erff of a few ulp, 2^-22 in all;
    where 1 + erff cancels (u = -10) the result is a zero beside the largest value's 40."""
    u = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 10.0, -10.0, 40.0, -40.0])
    x, w = torch.zeros(8, 4), torch.zeros(8, 4)
    x[:, 0], w[:, 0] = u, 1.0
    gemm = _Gemm(None, bn, layer=(x, w, torch.zeros(8), torch.zeros(8, 8), torch.ones(8)))
    got = gemm(1, False, None).cpu()
    print('gelu epilogue at', u.tolist(), '->', got[:, 0].tolist())
    assert torch.isfinite(got).all()
    assert torch.all(got[6] == 40.0) and torch.all(got[7] == 0.0)
    assert torch.all(got[:2] == 0.0) and torch.all(got[4] == 10.0)
    assert max_rel_err(got[:, 0], gelu_f64(u.double())) <= 2.0 ** -22


def test_vit_epilogue_rejects_what_it_does_not_support():
    from rick_amd import gemm_conv
    L = _lib()
    t = torch.zeros(1 << 14, device=DEV)
    p = t.data_ptr()
    ok = lambda: gemm_conv.descriptor(4, 1, 1, 64, (1, 1), (1, 1), (0, 0), 64, 64, [(p, 64, 0, 64)])      # noqa: E731
    assert L.lib.rick_inc_conv_vit_f32(p, p, p, None, None, 0, ok(), L.stream_ptr()) == 0
    assert L.lib.rick_inc_conv_vit_f32(p, p, p, p, None, 1, ok(), L.stream_ptr()) == 0
    assert L.lib.rick_inc_conv_vit_f32(p, p, p, None, None, 2, ok(), L.stream_ptr()) == 22               # unknown activation
    assert L.lib.rick_inc_conv_vit_f32(p, p, p, None, None, -1, ok(), L.stream_ptr()) == 22
    assert L.lib.rick_inc_conv_vit_f32(p, p, None, None, None, 0, ok(), L.stream_ptr()) == 22
    two = gemm_conv.descriptor(4, 1, 1, 64, (1, 1), (1, 1), (0, 0), 64, 64, [(p, 64, 0, 32), (p, 64, 32, 32)])
    assert L.lib.rick_inc_conv_vit_f32(p, p, p, None, None, 0, two, L.stream_ptr()) == 22                # nseg = 2: one destination only
    odd = gemm_conv.descriptor(4, 1, 1, 62, (1, 1), (1, 1), (0, 0), 64, 64, [(p, 64, 0, 64)])
    assert L.lib.rick_inc_conv_vit_f32(p, p, p, None, None, 0, odd, L.stream_ptr()) == 22                # K % 4
    torch.cuda.synchronize()


# ---- input kernel ---------------------------------------------------------------------------------------------------------
def input_images(h, w):
    return torch.rand(2, 3, h, w, generator=_gen(1000 * h + w)) * 2 - 1


def run_input(x, size, mean=None, std=None):
    """rick_vit_input_f32 with the constants, rick_clip_input_f32 without."""
    L = _lib()
    n, _, h, w = x.shape
    xd = x.to(DEV)
    out = torch.full((n + 1, size, size, 4), SENTINEL, device=DEV)              # one guard image behind the output
    if mean is None:
        L.check(L.lib.rick_clip_input_f32(xd.data_ptr(), out.data_ptr(), n, h, w, size, L.stream_ptr()), 'rick_clip_input_f32')
    else:
        L.check(L.lib.rick_vit_input_f32(xd.data_ptr(), out.data_ptr(), n, h, w, size, *mean, *std, L.stream_ptr()), 'rick_vit_input_f32')
    assert torch.all(out[n] == SENTINEL)
    return out[:n].cpu()


@pytest.mark.parametrize('hw', list(INPUT_CPU_BASE))
def test_input_kernel_with_clips_constants_is_clips_input_kernel(hw):
    x = input_images(*hw)
    assert torch.equal(run_input(x, 56, CLIP_MEAN, CLIP_STD), run_input(x, 56))


@pytest.mark.parametrize('hw', list(INPUT_CPU_BASE))
def test_input_kernel_with_imagenets_constants_vs_fp64(hw):
    x = input_images(*hw)
    ref = affine_f64(bicubic_f64(x, 56)).permute(0, 2, 3, 1)
    got = run_input(x, 56, MEAN, STD)
    err, base = max_rel_err(got[..., :3], ref), INPUT_CPU_BASE[hw]
    print(f'rick_vit_input_f32 {hw} -> 56: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.all(got[..., 3] == 0)
    assert torch.equal(run_input(x, 56, MEAN, STD), got)


def test_input_kernel_copies_at_the_output_size_and_rejects_bad_constants():
    L = _lib()
    x = input_images(56, 56)
    mean, std = (torch.tensor(v).view(1, 3, 1, 1) for v in (MEAN, STD))
    got = run_input(x, 56, MEAN, STD)
    assert torch.equal(got[..., :3], ((x * 0.5 + 0.5 - mean) / std).permute(0, 2, 3, 1))    # the affine alone, bit for bit
    t = torch.zeros(1 << 14, device=DEV)
    p, s = t.data_ptr(), L.stream_ptr()
    assert L.lib.rick_vit_input_f32(p, p, 1, 8, 8, 8, *MEAN, *STD, s) == 0
    for std_ in ((0.0, 0.2, 0.2), (0.2, -0.2, 0.2), (0.2, 0.2, math.nan), (0.2, math.inf, 0.2)):
        assert L.lib.rick_vit_input_f32(p, p, 1, 8, 8, 8, *MEAN, *std_, s) == 22
    assert L.lib.rick_vit_input_f32(p, p, 1, 8, 8, 8, math.nan, 0.4, 0.4, *STD, s) == 22
    assert L.lib.rick_vit_input_f32(None, p, 1, 8, 8, 8, *MEAN, *STD, s) == 22
    torch.cuda.synchronize()


# ---- tokens kernel --------------------------------------------------------------------------------------------------------
def test_tokens_kernel_is_one_rounded_add():
    L = _lib()
    N, T, C = 2, 17, 36
    g = _gen(77)
    patches, cls, pos = torch.randn(N, T - 1, C, generator=g), torch.randn(C, generator=g), torch.randn(T, C, generator=g)
    out = torch.full((N * T + 1, C), SENTINEL, device=DEV)
    dev = [v.to(DEV) for v in (patches, cls, pos)]
    L.check(L.lib.rick_vit_tokens_f32(*(v.data_ptr() for v in dev), out.data_ptr(), N, T, C, L.stream_ptr()), 'rick_vit_tokens_f32')
    assert torch.all(out[N * T] == SENTINEL)
    assert torch.equal(out[:N * T].cpu(), (torch.cat([cls.expand(N, 1, C), patches], 1) + pos).reshape(N * T, C))


def test_tokens_kernel_rejects_what_it_does_not_support():
    L = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    p, s = t.data_ptr(), L.stream_ptr()
    assert L.lib.rick_vit_tokens_f32(p, p, p, p, 2, 5, 16, s) == 0
    assert L.lib.rick_vit_tokens_f32(p, p, p, p, 0, 5, 16, s) == 0
    for N, T, C in ((2, 258, 16), (2, 1, 16), (2, 5, 18), (2, 5, 2052), (2, 5, 0), (-1, 5, 16)):
        assert L.lib.rick_vit_tokens_f32(p, p, p, p, N, T, C, s) == 22
    assert L.lib.rick_vit_tokens_f32(p, None, p, p, 2, 5, 16, s) == 22
    assert L.lib.rick_vit_tokens_f32(p + 4, p, p, p, 2, 5, 16, s) == 22       # 16-byte accesses
    torch.cuda.synchronize()


# ---- whole network --------------------------------------------------------------------------------------------------------
_NETS, _NET_REF = {}, {}


def network(name, layout='transformers'):
    from rick_amd.dinov2 import Dinov2Features
    if (name, layout) not in _NETS:
        cfg, heads = CONFIGS[name]
        _NETS[(name, layout)] = Dinov2Features.load(synthetic_dinov2_state_dict(cfg, 11, layout), device=DEV, batch=25, size=cfg['image'],
                                                    heads=heads)
    return _NETS[(name, layout)]


def network_inputs(name, px):
    return clip_images(27, px, seed=px + ord(name))


def network_reference(name, px):
    if (name, px) not in _NET_REF:
        cfg, heads = CONFIGS[name]
        _NET_REF[(name, px)] = features_f64(synthetic_dinov2_state_dict(cfg, 11), network_inputs(name, px), heads, cfg['image'])
    return _NET_REF[(name, px)]


@pytest.mark.parametrize('name,px,n', list(NET_CPU_BASE))
def test_network_vs_fp64(name, px, n):
    net = network(name)
    x = network_inputs(name, px)[:n].to(DEV)
    got = net(x)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, CONFIGS[name][0]['width']) and got.device.type == 'cuda'
    err, base = max_rel_err(got.cpu(), network_reference(name, px)[:n]), NET_CPU_BASE[(name, px, n)]
    print(f'DINOv2 {name} from {px}^2, n={n}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.equal(net(x), got)                                           # run to run


def test_the_launches_of_the_blocks_run_on_the_vit_epilogue():
    names = [(s.what, s.name) for s in network('A')._plan.tf.launches(3)]
    assert [n for w, n in names if w in ('out', 'fc', 'proj')] == ['rick_inc_conv_vit_f32'] * 6
    assert [n for w, n in names if w == 'qkv'] == ['rick_inc_conv_lin_f32'] * 2


@pytest.mark.parametrize('size', list(GOLDEN_CPU_BASE))
def test_network_on_the_golden_weights_vs_the_golden_outputs(size):
    """size 42: the checkpoint's 4 x 4 positional grid interpolated to 3 x 3."""
    from rick_amd.dinov2 import Dinov2Features
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    net = Dinov2Features.load(sd, device=DEV, size=size, heads=2)
    got = net(torch.from_numpy(z[f'images_{size}']).to(DEV))
    err, base = max_rel_err(got.cpu(), torch.from_numpy(z[f'pooler_output_{size}'])), GOLDEN_CPU_BASE[size]
    print(f'DINOv2 golden at {size}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base


@pytest.mark.parametrize('name,px', [('A', 56), ('B', 128)])
def test_both_layouts_give_the_same_bits(name, px):
    x = network_inputs(name, px)[:5].to(DEV)
    want = network(name)(x)
    for layout in ('original', 'transformers-prefixed'):
        assert torch.equal(network(name, layout)(x), want)


@pytest.mark.parametrize('name,px', [('A', 256), ('B', 128)])
def test_features_do_not_depend_on_the_batch(name, px):
    net = network(name)
    x = network_inputs(name, px).to(DEV)
    full = net(x)                                             # chunks of 25 + 2
    assert torch.equal(net(x[:1]), full[:1])                  # n = 1 against its row in n = 27
    assert torch.equal(net(x[24:27]), full[24:27])            # image 24: last of a chunk there, first of one here
    assert torch.equal(net(x[26:27]), full[26:27])
    assert torch.equal(net(x.flip(0)).flip(0), full)


def test_graph_capture_replays_the_eager_result():
    net = network('A')
    x = network_inputs('A', 256)
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
def test_evaluator_fd_and_kid_in_dinov2_space():
    from rick_amd.evaluate import Evaluator
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
    assert all(f.device.type == 'cuda' and f.dtype == torch.float32 and tuple(f.shape) == (16, 64) for f in seen)
    print(f"FD-DINOv2 {float(score['fid']):.4f}, KID {float(score['kid']):.5f}")
    assert math.isfinite(float(score['fid'])) and float(score['fid']) > 0
    assert math.isfinite(float(score['kid']))
