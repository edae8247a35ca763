"""CPU: the CLIP image tower's host side (rick_amd/clip.py): the fp64 restatement (tests/clip_f64.py) pinned to the golden
embeddings of an implementation the author did not write, the loader in both layouts, the packed GEMM operands restated, the
fp32 torch composition against the restatement, the resize rule, clip_similarity and the evaluator on CPU features.

Tolerances of the fp32 composition: its own error against the fp64 restatement, measured once here and written down below
(max error over the reference's max-norm), x 4 for another BLAS or thread count."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.clip_f64 import (SmoothG, affine_f64, bicubic_f64, clip_images, cubic_taps, embed_f64, max_rel_err,
                            synthetic_clip_state_dict)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clip_tiny.npz')
CFG = dict(width=64, patch=8, image=32, layers=2, mlp=256, dim=32)            # 4 heads of 16, T = 17
HEADS = 4
FACTOR = 4
# ClipImageFeatures on CPU tensors against the fp64 restatement: CFG with seed 11 on clip_images(3, size, size), and the golden
NET_CPU_BASE = {32: 5.857e-07, 64: 5.135e-07, 100: 4.151e-07}
GOLDEN_CPU_BASE = 2.510e-07


def golden():
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return sd, torch.from_numpy(z['images']), torch.from_numpy(z['image_embeds'])


def load(sd, **kw):
    from rick_amd.clip import ClipImageFeatures
    return ClipImageFeatures.load(sd, device='cpu', **kw)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_embeddings():
    sd, x, ref = golden()
    assert ref.dtype == torch.float64 and x.dtype == torch.float32 and all(v.dtype == torch.float32 for v in sd.values())
    err = max_rel_err(embed_f64(sd, x, 2), ref)
    print(f'fp64 restatement against the golden embeddings: {err:.3e}')
    assert err <= 1e-12


# ---- loader ---------------------------------------------------------------------------------------------------------------
def test_both_layouts_give_the_same_parameters_and_outputs():
    from rick_amd.clip import params_from_state_dict
    x = clip_images(3, 64, 1)
    want_p = params_from_state_dict(synthetic_clip_state_dict(CFG, 11))
    want = load(synthetic_clip_state_dict(CFG, 11), heads=HEADS)(x)
    for layout in ('openai', 'openai-visual'):
        sd = synthetic_clip_state_dict(CFG, 11, layout)
        p = params_from_state_dict(sd)
        assert p.keys() == want_p.keys() and all(torch.equal(p[k], want_p[k]) for k in p)
        assert all(v.dtype == torch.float32 and v.is_contiguous() for v in p.values())
        assert torch.equal(load(sd, heads=HEADS)(x), want)
    half = {k: v.half() for k, v in synthetic_clip_state_dict(CFG, 11, 'openai-visual').items()}      # OpenAI checkpoints are fp16
    p = params_from_state_dict(half)
    assert all(v.dtype == torch.float32 for v in p.values()) and torch.equal(p['cls'], want_p['cls'].half().float())


def test_text_tower_keys_are_ignored_and_unknown_keys_raise():
    want = load(synthetic_clip_state_dict(CFG, 11), heads=HEADS).params
    text = {'transformers': {'text_model.embeddings.token_embedding.weight': torch.zeros(5, 8), 'text_projection.weight': torch.zeros(4, 8),
                             'logit_scale': torch.tensor(4.6), 'vision_model.embeddings.position_ids': torch.arange(17)[None],
                             'text_model.embeddings.position_ids': torch.arange(7)[None]},
            'openai-visual': {'transformer.resblocks.0.ln_1.weight': torch.zeros(8), 'positional_embedding': torch.zeros(7, 8),
                              'token_embedding.weight': torch.zeros(5, 8), 'ln_final.bias': torch.zeros(8), 'text_projection': torch.zeros(8, 4),
                              'logit_scale': torch.tensor(4.6)},
            'openai': {'logit_scale': torch.tensor(4.6), 'token_embedding.weight': torch.zeros(5, 8)}}
    for layout, extra in text.items():
        sd = synthetic_clip_state_dict(CFG, 11, layout)
        got = load({**sd, **extra}, heads=HEADS).params
        assert all(torch.equal(got[k], want[k]) for k in want)
        unknown = ('vision_model.' if layout == 'transformers' else 'visual.' if layout == 'openai-visual' else '') + 'surprise.weight'
        with pytest.raises(RuntimeError, match='surprise'):
            load({**sd, unknown: torch.zeros(3)}, heads=HEADS)
        for key in list(sd)[::7]:
            with pytest.raises(RuntimeError, match='missing key'):
                load({k: v for k, v in sd.items() if k != key}, heads=HEADS)


def test_the_configuration_is_read_from_the_shapes():
    net = load(synthetic_clip_state_dict(CFG, 11, 'openai'), heads=HEADS)
    c = net.cfg
    assert (c.tokens, c.patch, c.size, c.layers, c.dim, c.heads, c.width, c.mlp, c.grid) == (17, 8, 32, 2, 32, 4, 64, 256, 4)
    assert load(synthetic_clip_state_dict(CFG, 11)).cfg.heads == 1            # CLIP's rule: width / 64
    sd, _, _ = golden()
    g = load(sd, heads=2).cfg
    assert (g.tokens, g.patch, g.size, g.layers, g.dim, g.heads, g.width, g.mlp) == (17, 8, 32, 2, 16, 2, 32, 128)


def test_unsupported_configurations_are_refused_at_load():
    sd = synthetic_clip_state_dict(CFG, 11)
    for heads in (8, 3, 0):                                                   # head dim 8; no divisor; nonsense
        with pytest.raises(RuntimeError, match='head'):
            load(sd, heads=heads)
    with pytest.raises(RuntimeError, match='multiple of 64'):
        load(synthetic_clip_state_dict({**CFG, 'width': 32}, 11))            # no heads= and width / 64 is no integer
    pos = 'vision_model.embeddings.position_embedding.weight'
    with pytest.raises(RuntimeError, match='258 tokens'):
        load({**sd, pos: torch.zeros(258, 64)}, heads=HEADS)                  # one token past ViT-L/14 at 224
    with pytest.raises(RuntimeError, match='tokens|G\\^2'):
        load({**sd, pos: torch.zeros(290, 64)}, heads=HEADS)                  # 17^2 + 1
    with pytest.raises(RuntimeError, match='G\\^2'):
        load({**sd, pos: torch.zeros(18, 64)}, heads=HEADS)
    with pytest.raises(RuntimeError):
        load(synthetic_clip_state_dict({**CFG, 'width': 66}, 11), heads=HEADS)


# ---- GEMM operands --------------------------------------------------------------------------------------------------------
def test_packed_operands_of_the_patch_embedding_and_of_qkv():
    """The layout rick_inc_conv_lin_f32 reads, restated: row (ky, kx, c) of the NHWC4 input with a zero row for c = 3, column =
    output feature; K rounded up to 32 rows, columns to the block, padding zero.  q, k, v rows of the transformers layout land
    in column blocks [0, Wd), [Wd, 2 Wd), [2 Wd, 3 Wd)."""
    from rick_amd.clip import pack_linear, pack_patch_embedding, params_from_state_dict
    sd = synthetic_clip_state_dict({**CFG, 'width': 36, 'patch': 5, 'image': 20}, 3)      # K = 100 and 36: neither a multiple of 32
    p = params_from_state_dict(sd)
    w = sd['vision_model.embeddings.patch_embedding.weight']
    wpk, bias, cop, bn = pack_patch_embedding(w)
    assert bn == 64 and cop == 64 and tuple(wpk.shape) == (128, 64) and torch.all(bias == 0)
    want = torch.zeros(128, 64)
    for ky in range(5):
        for kx in range(5):
            for c in range(3):
                want[(ky * 5 + kx) * 4 + c, :36] = w[:, c, ky, kx]
    assert torch.equal(wpk, want)
    pre = 'vision_model.encoder.layers.1.self_attn.'
    wpk, bias, cop, bn = pack_linear(p['blocks.1.qkv.w'], p['blocks.1.qkv.b'])
    assert bn == 128 and cop == 128 and tuple(wpk.shape) == (64, 128)         # 108 columns pad least in one block of 128
    want, want_b = torch.zeros(64, 128), torch.zeros(128)
    for j, name in enumerate('qkv'):
        want[:36, 36 * j:36 * (j + 1)] = sd[f'{pre}{name}_proj.weight'].T
        want_b[36 * j:36 * (j + 1)] = sd[f'{pre}{name}_proj.bias']
    assert torch.equal(wpk, want) and torch.equal(bias, want_b)


# ---- the fp32 composition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', list(NET_CPU_BASE))
def test_cpu_path_vs_fp64(size):
    sd = synthetic_clip_state_dict(CFG, 11)
    x = clip_images(3, size, size)
    got = load(sd, heads=HEADS, batch=2)(x)                                   # chunks of 2 + 1
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 32)
    err, base = max_rel_err(got, embed_f64(sd, x, HEADS)), NET_CPU_BASE[size]
    print(f'CLIP on the CPU from {size}^2: max err / max-norm {err:.3e} (measured {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base


def test_cpu_path_on_the_golden():
    sd, x, ref = golden()
    err = max_rel_err(load(sd, heads=2)(x), ref)
    print(f'CLIP on the CPU, golden: {err:.3e} (measured {GOLDEN_CPU_BASE:.3e}, bound {FACTOR * GOLDEN_CPU_BASE:.3e})')
    assert err <= FACTOR * GOLDEN_CPU_BASE


@pytest.mark.parametrize('hw,size', [((256, 256), 224), ((64, 64), 224), ((299, 299), 224), ((100, 317), 224), ((40, 33), 32)])
def test_interpolate_bicubic_is_the_restated_rule(hw, size):
    """F.interpolate(mode='bicubic', align_corners=False) against the restated index and weight rule with the positions formed
    in fp32 like ATen's.  Two things are left.  The rounding of the weights, products and sums: each output is a sum of terms
    bounded by sum|wy| sum|wx| max|x| <= 1.375^2 (the weights' absolute sum peaks at t = 0.5: 2 (0.59375 + 0.09375)); 40
    roundings of 2^-24 on that scale bound it generously.  And one ulp of the fp32 source position per axis (an fma or another
    order of the same expression): a position below n_in has an ulp of at most 2^-23 2^floor(log2 n_in), and the interpolant's
    slope is at most sum|w'| sum|w| max|x| <= 4.2 x 1.375 (|w'| <= 1.35 for the inner taps, 0.75 for the outer ones)."""
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(hw[1])) * 2 - 1
    got = F.interpolate(x, size=(size, size), mode='bicubic', align_corners=False)
    (iy, wy), (ix, wx) = cubic_taps(hw[0], size, torch.float32), cubic_taps(hw[1], size, torch.float32)
    rows = (x.double()[:, :, :, ix] * wx.double()).sum(-1)
    want = (rows[:, :, iy] * wy.double()[:, :, None]).sum(3)
    err = float((got.double() - want).abs().max())
    print(f'F.interpolate bicubic {hw} -> {size}: max abs difference {err:.3e}')
    ulps = sum(2.0 ** (-23 + math.floor(math.log2(n))) for n in hw)
    assert err <= 40 * 2.0 ** -24 * 1.375 ** 2 + 4.2 * 1.375 * ulps
    assert float(wy.abs().sum(1).max()) <= 1.375 + 1e-6
    assert float((bicubic_f64(x, size) - want).abs().max()) < 1e-4            # fp64 positions move the taps by ~1e-5 pixel


def test_cpu_path_copies_at_the_network_size():
    from rick_amd.clip import MEAN, STD, resize_affine
    x = clip_images(3, 32, 2)
    mean, std = (torch.tensor(v).view(1, 3, 1, 1) for v in (MEAN, STD))
    assert torch.equal(resize_affine(x, 32), (x * 0.5 + 0.5 - mean) / std)
    iy, wy = cubic_taps(32, 32, torch.float32)
    assert torch.equal(wy, torch.tensor([0.0, 1.0, 0.0, 0.0]).expand(32, 4))
    assert max_rel_err(resize_affine(x, 32), affine_f64(x)) < 1e-6


# ---- similarity and the evaluator -----------------------------------------------------------------------------------------
def test_clip_similarity_vs_direct_fp64():
    from rick_amd.evaluate import clip_similarity
    g = torch.Generator().manual_seed(0)
    fa, fb = torch.randn(5, 16, generator=g), torch.randn(7, 16, generator=g) * 3
    got = clip_similarity(fa, fb)
    assert got.dtype == torch.float64 and tuple(got.shape) == (5, 7)
    for i in range(5):
        for j in range(7):
            a, b = fa[i].double(), fb[j].double()
            assert abs(float(got[i, j]) - float((a * b).sum() / math.sqrt(float((a * a).sum()) * float((b * b).sum())))) < 1e-14
    assert torch.allclose(clip_similarity(fa, fa).diagonal(), torch.ones(5, dtype=torch.float64), atol=1e-14)
    with pytest.raises(RuntimeError):
        clip_similarity(fa, fb[:, :8])


def test_evaluator_takes_the_cpu_network_as_feature_fn():
    from rick_amd.evaluate import Evaluator
    net = load(synthetic_clip_state_dict(CFG, 11), heads=HEADS, batch=5)
    g = SmoothG(32)
    seen = []

    def feature_fn(img):
        f = net(img)
        seen.append(f)
        return f
    real = net(clip_images(48, 32, 5))
    ev = Evaluator(g, feature_fn, real, n_sample_store=16, inception_nsamples=48, fid_sample_size=48)
    z = torch.randn(48, 512, generator=torch.Generator().manual_seed(39))
    score = ev.compute_inception_score(fid=True, kid=True, latents=z, kid_subsets=4, kid_subset_size=24, rng=np.random.RandomState(0))
    assert len(seen) == 3 and all(f.dtype == torch.float32 and tuple(f.shape) == (16, 32) for f in seen)
    print(f"CLIP-space FID {float(score['fid']):.4f}, KID {float(score['kid']):.5f}")
    assert math.isfinite(float(score['fid'])) and float(score['fid']) > 0
    assert math.isfinite(float(score['kid']))
