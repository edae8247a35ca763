"""CPU: the host side of DINOv2's ViT (rick_amd/dinov2.py): the fp64 restatement (tests/dinov2_f64.py) pinned to the golden
outputs of an implementation the author did not write (with and without the interpolated positional embedding), the loader in
both layouts and everything it refuses, the size limits, the fp32 torch composition against the restatement, and the shared
transformer's CLIP side (rick_amd/cliptower.py) called as before the blocks took their differences as data.

Tolerances of the fp32 composition: its own error against the fp64 restatement, measured once here and written down below
(max error over the reference's max-norm), x 4 for another BLAS or thread count."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.clip_f64 import synthetic_clip_state_dict
from tests.dinov2_f64 import SmoothG, clip_images, features_f64, max_rel_err, pos_f64, synthetic_dinov2_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dinov2_tiny.npz')
CFG = dict(width=64, patch=14, image=56, layers=2, mlp=256)                   # 4 heads of 16, T = 17
HEADS = 4
FACTOR = 4
# The restatement against the golden outputs.  At 56 both sides are fp64 throughout: the bound of tests/test_clip.py.  At 42
# the library that wrote the golden interpolates the positional embedding in fp32 whatever the model's dtype and the
# restatement does it in fp64: the difference measured here, x 4.
RESTATEMENT_BOUND = {56: 1e-12, 42: FACTOR * 6.673e-08}
# Dinov2Features on CPU tensors against the fp64 restatement: CFG with seed 11 on clip_images(3, px, px) at (size, px), and the
# golden at either size
NET_CPU_BASE = {(56, 56): 3.547e-07, (56, 100): 5.918e-07, (42, 64): 5.551e-07}
GOLDEN_CPU_BASE = {56: 1.195e-06, 42: 5.328e-07}
BLOCKS_CPU_BASE = 3.057e-07                                                  # torch_blocks alone: CFG's two layers on 2 x 17 x 64 normals


def golden(size):
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return sd, torch.from_numpy(z[f'images_{size}']), torch.from_numpy(z[f'pooler_output_{size}'])


def load(sd, **kw):
    from rick_amd.dinov2 import Dinov2Features
    return Dinov2Features.load(sd, device='cpu', **kw)


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [56, 42])
def test_restatement_reproduces_the_golden_outputs(size):
    sd, x, ref = golden(size)
    assert ref.dtype == torch.float64 and x.dtype == torch.float32 and all(v.dtype == torch.float32 for v in sd.values())
    assert tuple(x.shape) == (3, 3, size, size) and tuple(sd['embeddings.position_embeddings'].shape) == (1, 17, 32)
    err = max_rel_err(features_f64(sd, x, 2, size), ref)
    print(f'fp64 restatement against the golden outputs at {size}: {err:.3e} (bound {RESTATEMENT_BOUND[size]:.3e})')
    assert err <= RESTATEMENT_BOUND[size]


@pytest.mark.parametrize('g,grid', [(4, 3), (4, 4), (3, 7), (37, 16)])
def test_positional_embedding_is_interpolated_by_the_restated_rule(g, grid):
    """interpolate_pos (F.interpolate in fp32) against the written rule in fp64.  A value is a sum of 16 products of weights with
    an absolute sum of at most 1.375^2 (tests/test_clip.py); 40 roundings of 2^-24 on that scale bound the arithmetic, and one
    ulp of the fp32 source position per axis moves the interpolant by at most 4.2 x 1.375 per unit."""
    from rick_amd.dinov2 import interpolate_pos
    pos = torch.randn(g * g + 1, 8, generator=torch.Generator().manual_seed(g))
    got = interpolate_pos(pos, grid)
    assert tuple(got.shape) == (grid * grid + 1, 8) and got.dtype == torch.float32 and torch.equal(got[0], pos[0])
    if g == grid:
        assert got is pos
    scale = float(pos.abs().max())
    ulps = 2 * 2.0 ** (-23 + math.floor(math.log2(g)))
    assert float((got.double() - pos_f64(pos.double(), grid)).abs().max()) <= scale * (40 * 2.0 ** -24 * 1.375 ** 2 + 4.2 * 1.375 * ulps)


# ---- loader ---------------------------------------------------------------------------------------------------------------
def test_both_layouts_give_the_same_parameters_and_outputs():
    from rick_amd.dinov2 import params_from_state_dict
    x = clip_images(3, 64, 1)
    want_p = params_from_state_dict(synthetic_dinov2_state_dict(CFG, 11))
    want = load(synthetic_dinov2_state_dict(CFG, 11), heads=HEADS, size=56)(x)
    assert tuple(want_p['pos'].shape) == (17, 64) and tuple(want_p['cls'].shape) == (64,) and tuple(want_p['blocks.1.ls2'].shape) == (64,)
    for layout in ('original', 'transformers-prefixed'):
        sd = synthetic_dinov2_state_dict(CFG, 11, layout)
        p = params_from_state_dict(sd)
        assert p.keys() == want_p.keys() and all(torch.equal(p[k], want_p[k]) for k in p)
        assert all(v.dtype == torch.float32 and v.is_contiguous() for v in p.values())
        assert torch.equal(load(sd, heads=HEADS, size=56)(x), want)
    half = {k: v.half() for k, v in synthetic_dinov2_state_dict(CFG, 11, 'original').items()}
    p = params_from_state_dict(half)
    assert all(v.dtype == torch.float32 for v in p.values()) and torch.equal(p['cls'], want_p['cls'].half().float())


def test_the_configuration_is_read_from_the_shapes():
    c = load(synthetic_dinov2_state_dict(CFG, 11, 'original'), heads=HEADS, size=56).cfg
    assert (c.tokens, c.patch, c.size, c.layers, c.heads, c.width, c.mlp, c.grid, c.dim) == (17, 14, 56, 2, 4, 64, 256, 4, 64)
    assert load(synthetic_dinov2_state_dict(CFG, 11), size=56).cfg.heads == 1                  # width / 64
    net = load(synthetic_dinov2_state_dict(CFG, 11), heads=HEADS, size=98)                     # 4 x 4 -> 7 x 7
    assert (net.cfg.tokens, net.cfg.grid) == (50, 7) and tuple(net.params['pos'].shape) == (50, 64)
    sd, _, _ = golden(56)
    g = load(sd, heads=2, size=42).cfg
    assert (g.tokens, g.patch, g.size, g.layers, g.heads, g.width, g.mlp) == (10, 14, 42, 2, 2, 32, 128)


def test_registers_swiglu_and_unknown_keys_are_refused_by_name():
    for layout in ('transformers', 'transformers-prefixed', 'original'):
        sd = synthetic_dinov2_state_dict(CFG, 11, layout)
        v = 'dinov2.' if layout == 'transformers-prefixed' else ''
        hf = layout != 'original'
        reg = v + 'embeddings.register_tokens' if hf else 'register_tokens'
        with pytest.raises(RuntimeError, match='Dinov2Features.*register_tokens'):
            load({**sd, reg: torch.zeros(1, 4, 64)}, heads=HEADS, size=56)
        swiglu = (v + 'encoder.layer.0.mlp.weights_in.weight') if hf else 'blocks.0.mlp.w12.weight'
        fc1 = (v + 'encoder.layer.0.mlp.fc1.') if hf else 'blocks.0.mlp.fc1.'
        giant = {k: t for k, t in sd.items() if not k.startswith(fc1)}
        with pytest.raises(RuntimeError, match='Dinov2Features.*' + swiglu.replace('.', '\\.')):
            load({**giant, swiglu: torch.zeros(512, 64)}, heads=HEADS, size=56)
        unknown = v + 'surprise.weight'
        with pytest.raises(RuntimeError, match='Dinov2Features.*surprise'):
            load({**sd, unknown: torch.zeros(3)}, heads=HEADS, size=56)
        for key in list(sd)[::7]:
            if 'mask_token' in key or key.startswith('classifier.'):
                continue
            with pytest.raises(RuntimeError, match='Dinov2Features.*missing key'):
                load({k: t for k, t in sd.items() if k != key}, heads=HEADS, size=56)
    sd = synthetic_dinov2_state_dict(CFG, 11)
    got = load({k: t for k, t in sd.items() if 'mask_token' not in k}, heads=HEADS, size=56).params      # ignored, so not needed
    want = load(sd, heads=HEADS, size=56).params
    assert all(torch.equal(got[k], want[k]) for k in want)


def test_sizes_and_grids_that_are_not_supported_are_refused():
    sd = synthetic_dinov2_state_dict(CFG, 11)
    with pytest.raises(RuntimeError, match='Dinov2Features.*multiple of the patch size'):
        load(sd, heads=HEADS, size=60)
    with pytest.raises(RuntimeError, match='Dinov2Features.*290 tokens'):
        load(sd, heads=HEADS, size=238)                                       # 17^2 + 1
    pos = 'embeddings.position_embeddings'
    for rows in (18, 13, 1):                                                  # no square grid behind the class row
        with pytest.raises(RuntimeError, match='Dinov2Features.*G\\^2'):
            load({**sd, pos: torch.zeros(1, rows, 64)}, heads=HEADS, size=56)
    with pytest.raises(RuntimeError, match='Dinov2Features.*position_embeddings'):
        load({**sd, pos: torch.zeros(17, 64)}, heads=HEADS, size=56)
    for heads in (8, 3, 0):                                                   # head dim 8; no divisor; nonsense
        with pytest.raises(RuntimeError, match='head'):
            load(sd, heads=heads, size=56)
    with pytest.raises(ValueError):
        load(sd, heads=HEADS, size=56, batch=0)


def test_a_518_pixel_checkpoint_loads_at_224_and_not_at_238():
    """The released checkpoints carry a 37 x 37 grid (518 px): 224 px is 16^2 + 1 = 257 tokens, the kernels' limit."""
    sd = synthetic_dinov2_state_dict(dict(width=64, patch=14, image=518, layers=1, mlp=64), 5)
    assert tuple(sd['embeddings.position_embeddings'].shape) == (1, 1370, 64)
    net = load(sd)                                                            # size 224 and heads = width / 64 by default
    assert (net.cfg.tokens, net.cfg.grid, net.cfg.size, net.cfg.heads) == (257, 16, 224, 1) and tuple(net.params['pos'].shape) == (257, 64)
    with pytest.raises(RuntimeError, match='Dinov2Features.*290 tokens'):
        load(sd, size=238)


# ---- the fp32 composition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size,px', list(NET_CPU_BASE))
def test_cpu_path_vs_fp64(size, px):
    sd = synthetic_dinov2_state_dict(CFG, 11)
    x = clip_images(3, px, px)
    got = load(sd, heads=HEADS, batch=2, size=size)(x)                        # chunks of 2 + 1
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 64)
    err, base = max_rel_err(got, features_f64(sd, x, HEADS, size)), NET_CPU_BASE[(size, px)]
    print(f'DINOv2 on the CPU at {size} from {px}^2: max err / max-norm {err:.3e} (measured {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base


@pytest.mark.parametrize('size', [56, 42])
def test_cpu_path_on_the_golden(size):
    sd, x, ref = golden(size)
    err = max_rel_err(load(sd, heads=2, size=size)(x), ref)
    print(f'DINOv2 on the CPU, golden at {size}: {err:.3e} (measured {GOLDEN_CPU_BASE[size]:.3e}, bound {FACTOR * GOLDEN_CPU_BASE[size]:.3e})')
    assert err <= FACTOR * GOLDEN_CPU_BASE[size]


def test_evaluator_takes_the_cpu_network_as_feature_fn():
    from rick_amd.evaluate import Evaluator
    net = load(synthetic_dinov2_state_dict(CFG, 11), heads=HEADS, batch=5, size=56)
    real = net(clip_images(48, 32, 5))
    ev = Evaluator(SmoothG(32), net, real, n_sample_store=16, inception_nsamples=48, fid_sample_size=48)
    z = torch.randn(48, 512, generator=torch.Generator().manual_seed(39))
    score = ev.compute_inception_score(fid=True, kid=True, latents=z, kid_subsets=4, kid_subset_size=24, rng=np.random.RandomState(0))
    print(f"FD-DINOv2 {float(score['fid']):.4f}, KID {float(score['kid']):.5f}")
    assert math.isfinite(float(score['fid'])) and float(score['fid']) > 0
    assert math.isfinite(float(score['kid']))


# ---- the shared transformer, CLIP's side ----------------------------------------------------------------------------------
CLIP_CFG = dict(width=64, patch=8, image=32, layers=2, mlp=256, dim=32)


def _clip_blocks_as_they_were(p, cfg, t, mask=None):
    """rick_amd.cliptower.torch_blocks as it stood before the blocks took eps, activation and LayerScale as data."""
    wd, d, T = cfg.width, cfg.width // cfg.heads, cfg.tokens
    n = t.shape[0]
    for i in range(cfg.layers):
        b = f'blocks.{i}.'
        h = F.layer_norm(t, (wd,), p[b + 'ln1.w'], p[b + 'ln1.b'], 1e-5)
        q, k, v = (u.view(n, T, cfg.heads, d).transpose(1, 2) for u in F.linear(h, p[b + 'qkv.w'], p[b + 'qkv.b']).split(wd, 2))
        s = q @ k.transpose(2, 3) * (1.0 / math.sqrt(d))
        a = torch.softmax(s if mask is None else s + mask, -1) @ v
        t = t + F.linear(a.transpose(1, 2).reshape(n, T, wd), p[b + 'out.w'], p[b + 'out.b'])
        h = F.linear(F.layer_norm(t, (wd,), p[b + 'ln2.w'], p[b + 'ln2.b'], 1e-5), p[b + 'fc.w'], p[b + 'fc.b'])
        t = t + F.linear(h * torch.sigmoid(1.702 * h), p[b + 'proj.w'], p[b + 'proj.b'])
    return t


def test_clips_loaders_and_blocks_keep_their_signatures_and_results():
    from rick_amd.clip import config_from_params, params_from_state_dict
    from rick_amd.cliptower import blocks_from_state_dict, torch_blocks
    hf, openai = synthetic_clip_state_dict(CLIP_CFG, 11), synthetic_clip_state_dict(CLIP_CFG, 11, 'openai')
    a, used_a = blocks_from_state_dict(hf, 'vision_model.encoder.layers.', True, 64, 'test')       # five positional arguments
    b, used_b = blocks_from_state_dict(openai, 'transformer.resblocks.', False, 64, 'test')
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a) and not any('ls' in k for k in a)
    assert sorted(a) == sorted(f'blocks.{i}.{n}.{s}' for i in range(2) for n in ('ln1', 'qkv', 'out', 'ln2', 'fc', 'proj') for s in 'wb')
    assert used_a == {k for k in hf if '.layers.' in k} and used_b == {k for k in openai if '.resblocks.' in k}
    for i in range(2):
        pre = f'vision_model.encoder.layers.{i}.'
        assert torch.equal(a[f'blocks.{i}.qkv.w'], torch.cat([hf[f'{pre}self_attn.{n}_proj.weight'] for n in 'qkv']))
        assert torch.equal(a[f'blocks.{i}.qkv.b'], openai[f'transformer.resblocks.{i}.attn.in_proj_bias'])
        assert torch.equal(a[f'blocks.{i}.fc.w'], hf[pre + 'mlp.fc1.weight']) and torch.equal(a[f'blocks.{i}.ln2.b'], hf[pre + 'layer_norm2.bias'])
    p = params_from_state_dict(hf)
    cfg = config_from_params(p, 4)
    t = torch.randn(3, 17, 64, generator=torch.Generator().manual_seed(2))
    mask = torch.full((17, 17), -math.inf).triu(1)
    assert torch.equal(torch_blocks(p, cfg, t), _clip_blocks_as_they_were(p, cfg, t))
    assert torch.equal(torch_blocks(p, cfg, t, mask), _clip_blocks_as_they_were(p, cfg, t, mask))
    with pytest.raises(RuntimeError, match='activation'):
        torch_blocks(p, cfg, t, act='relu')


def test_the_blocks_take_eps_activation_and_layerscale_as_data():
    """torch_blocks with DINOv2's data against a composition written out here, one layer at a time."""
    from rick_amd.dinov2 import config_from_params, params_from_state_dict
    from rick_amd.cliptower import torch_blocks
    p = params_from_state_dict(synthetic_dinov2_state_dict(CFG, 11))
    cfg = config_from_params(p, 56, HEADS)
    t = torch.randn(2, 17, 64, generator=torch.Generator().manual_seed(4))
    got = torch_blocks(p, cfg, t, eps=1e-6, act='gelu')
    assert not torch.equal(got, torch_blocks(p, cfg, t, eps=1e-6))            # QuickGELU is another function
    no_ls = {k: v for k, v in p.items() if '.ls' not in k}
    ones = {**p, **{k: torch.ones_like(v) for k, v in p.items() if '.ls' in k}}
    assert torch.equal(torch_blocks(no_ls, cfg, t, eps=1e-6, act='gelu'), torch_blocks(ones, cfg, t, eps=1e-6, act='gelu'))
    want = t.double()
    for i in range(2):
        g = lambda k: p[f'blocks.{i}.{k}'].double()                           # noqa: E731,B023
        h = F.layer_norm(want, (64,), g('ln1.w'), g('ln1.b'), 1e-6)
        q, k, v = (u.view(2, 17, 4, 16).transpose(1, 2) for u in F.linear(h, g('qkv.w'), g('qkv.b')).split(64, 2))
        a = (torch.softmax(q @ k.transpose(2, 3) / 4.0, -1) @ v).transpose(1, 2).reshape(2, 17, 64)
        want = want + g('ls1') * F.linear(a, g('out.w'), g('out.b'))
        u = F.linear(F.layer_norm(want, (64,), g('ln2.w'), g('ln2.b'), 1e-6), g('fc.w'), g('fc.b'))
        want = want + g('ls2') * F.linear(0.5 * u * (1 + torch.erf(u / math.sqrt(2.0))), g('proj.w'), g('proj.b'))
    err = max_rel_err(got, want)
    print(f'torch_blocks with DINOv2\'s data against fp64: {err:.3e} (measured {BLOCKS_CPU_BASE:.3e}, bound {FACTOR * BLOCKS_CPU_BASE:.3e})')
    assert err <= FACTOR * BLOCKS_CPU_BASE
