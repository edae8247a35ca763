"""CPU: the gradient side of the CLIP image tower.  The hand-written fp64 adjoints of tests/clip_grad_f64.py (the references of
the GPU kernel tests) against torch fp64 autograd of the forward restatement; torch autograd of the restatement
(tests/clip_f64.embed_f64) against the gradient golden of an implementation the author did not write; ``encode`` on CPU
tensors; the CLIP-space loss heads against fp64 formulas, gradients included; the trainer's validation of the new fields."""
import math
import os

import numpy as np
import pytest
import torch

from tests import clip_grad_f64 as R
from tests.clip_f64 import affine_f64, bicubic_f64, clip_images, embed_f64, max_rel_err, synthetic_clip_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CFG_A, HEADS_A = dict(width=64, patch=8, image=32, layers=2, mlp=256, dim=32), 4     # config A of tests/test_gpu_clip.py
F64 = 1e-12                      # two fp64 evaluations of one formula in different orders, values O(1) to O(100)
# embed_f64's autograd gradient against the golden's (transformers in fp64): measured 9.8e-16 of the max-norm, the forward
# agrees to 5e-16; the bound leaves two decimal digits for another BLAS's summation order
GOLDEN_GRAD_AGREEMENT = 1e-14
# ClipImageFeatures.encode on CPU tensors (fp32 torch autograd) against embed_f64's autograd on network A from 32^2, n = 3:
# measured 3.6e-07 (tests/test_gpu_clip_grad.py NET_GRAD_CPU_BASE); fp32 against fp64, so the bound is that figure x 4
ENCODE_CPU_BOUND = 4 * 3.593e-07


def _autograd(fn, x, g):
    x = x.double().requires_grad_()
    fn(x).backward(g.double())
    return x.grad


# ---- the helper's adjoints equal fp64 autograd of the forward restatement ---------------------------------------------------
def test_quickgelu_adjoint_is_autograd_of_the_restatement():
    u, g = R.quickgelu_bwd_inputs()
    ref = _autograd(lambda v: v / (1 + torch.exp(-1.702 * v)), u, g)
    assert max_rel_err(R.quickgelu_grad_f64(u, g), ref) <= F64


@pytest.mark.parametrize('R_,C,offset', [(51, 64, False), (5, 36, False), (51, 768, True)])
def test_layernorm_adjoint_is_autograd_of_the_restatement(R_, C, offset):
    from tests.clip_f64 import _ln
    x, w, g = R.layernorm_bwd_inputs(R_, C, offset)
    ref = _autograd(lambda v: _ln(v, w.double(), torch.zeros(C, dtype=torch.float64)), x, g)
    assert float(ref.abs().max()) > 0
    assert max_rel_err(R.layernorm_grad_f64(x, w, g), ref) <= (1e-9 if offset else F64)     # mean 100: cancellation in fp64 too


def test_tokens_adjoint_is_autograd_of_the_restatement():
    from tests.clip_f64 import _ln
    patches, pos, w, g = R.tokens_bwd_inputs()
    cls = torch.randn(64, dtype=torch.float64, generator=torch.Generator().manual_seed(1))

    def fwd(p):
        return _ln(torch.cat([cls.expand(3, 1, 64), p], 1) + pos.double(), w.double(), torch.zeros(64, dtype=torch.float64))
    assert max_rel_err(R.tokens_grad_f64(patches, pos, w, g), _autograd(fwd, patches, g)) <= F64


@pytest.mark.parametrize('T,d,heads,qscale', [(17, 16, 4, 1.0), (17, 16, 4, 30.0), (50, 64, 2, 1.0)])
def test_attention_adjoint_is_autograd_of_the_restatement(T, d, heads, qscale):
    qkv, go = R.attention_bwd_inputs(T, d, heads, qscale)

    def fwd(x):                                               # embed_f64's attention, one image and one head at a time
        out = []
        for im in x:
            q, k, v = im.reshape(T, 3, heads * d).unbind(1)
            att = []
            for hd in range(heads):
                c = slice(hd * d, (hd + 1) * d)
                s = q[:, c] @ k[:, c].T / math.sqrt(d)
                e = torch.exp(s - s.max(1, keepdim=True).values)
                att.append((e / e.sum(1, keepdim=True)) @ v[:, c])
            out.append(torch.cat(att, 1))
        return torch.stack(out)
    ref = _autograd(fwd, qkv, go)
    assert float(ref.abs().max()) > 0
    assert max_rel_err(R.attention_grad_f64(qkv, go, d, heads), ref) <= F64


@pytest.mark.parametrize('hw', [(64, 64), (100, 317), (40, 23), (32, 32)])
def test_input_adjoint_is_autograd_of_the_restatement(hw):
    g = R.input_bwd_inputs(32 if hw == (32, 32) else 56)
    ref = R.input_bwd_autograd_f64(g, *hw)
    assert float(ref.abs().max()) > 0
    assert max_rel_err(R.input_grad_f64(g, *hw), ref) <= F64
    x = torch.rand(2, 3, *hw, dtype=torch.float64)           # and the adjoint identity <A x, g> = <x, A^T g>, A the linear part
    lin = affine_f64(bicubic_f64(x, g.shape[-1])) - affine_f64(bicubic_f64(torch.zeros_like(x), g.shape[-1]))
    assert abs(float((lin * g).sum() - (x * ref).sum())) <= 1e-10 * float((lin * g).abs().sum())


def test_patch_rows_layout():
    g = R.input_bwd_inputs(32)
    rows = R.patch_rows(g, 8).view(2, 4, 4, 8, 8, 4)         # (n, gy, gx, ky, kx, c)
    assert float(rows[1, 2, 3, 5, 6, 1]) == float(g[1, 1, 2 * 8 + 5, 3 * 8 + 6]) and torch.all(rows[..., 3] == 7)


# ---- the restatement's gradient against an implementation the author did not write ------------------------------------------
def test_restatement_gradient_vs_the_golden():
    z, zg = np.load(os.path.join(GOLDEN, 'clip_tiny.npz')), np.load(os.path.join(GOLDEN, 'clip_tiny_grad.npz'))
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    x = torch.from_numpy(z['images']).double().requires_grad_()
    (grad,) = torch.autograd.grad((embed_f64(sd, x, 2) * torch.from_numpy(zg['r'])).sum(), x)
    ref = torch.from_numpy(zg['grad'])
    assert ref.dtype == torch.float64 and float(ref.abs().max()) > 0
    err = max_rel_err(grad, ref)
    print(f'embed_f64 autograd against the golden gradient: {err:.3e}')
    assert err <= GOLDEN_GRAD_AGREEMENT


# ---- encode on CPU tensors ------------------------------------------------------------------------------------------------------
def _net_a():
    from rick_amd.clip import ClipImageFeatures
    return ClipImageFeatures.load(synthetic_clip_state_dict(CFG_A, 11), device='cpu', heads=HEADS_A)


def test_encode_on_cpu_tensors():
    net = _net_a()
    x = clip_images(27, 32, seed=32 + ord('A'))[:3]          # network_inputs('A', 32)[:3] of the GPU tests
    r = R.network_upstream(3, 32)
    assert torch.equal(net.encode(x), net(x)) and not net.encode(x).requires_grad
    xg = x.clone().requires_grad_()
    emb = net.encode(xg)
    assert emb.requires_grad and torch.equal(emb.detach(), net(x))
    (g,) = torch.autograd.grad((emb * r).sum(), xg)
    x64 = x.double().requires_grad_()
    (ref,) = torch.autograd.grad((embed_f64(synthetic_clip_state_dict(CFG_A, 11), x64, HEADS_A) * r.double()).sum(), x64)
    assert float(ref.abs().max()) > 0
    err = max_rel_err(g, ref)
    print(f'encode on CPU tensors: gradient against fp64 {err:.3e}')
    assert err <= ENCODE_CPU_BOUND
    with torch.no_grad():
        assert not net.encode(xg).requires_grad
    with pytest.raises(RuntimeError, match='prepare_grad needs a network loaded for a GPU'):
        net.prepare_grad()


def test_transposed_operands():
    """pack_linear_transposed: the operand of gx = gy W; pack_patch_embedding_transposed: pack_patch_embedding's operand,
    transposed."""
    from rick_amd.clip import pack_linear, pack_linear_transposed, pack_patch_embedding, pack_patch_embedding_transposed
    gen = torch.Generator().manual_seed(4)
    w = torch.randn(40, 72, generator=gen)
    wt, bias, cop, bn = pack_linear_transposed(w)
    assert (cop, bn) == (128, 128) and wt.shape == (64, 128) and not bias.any()
    assert torch.equal(wt[:40, :72], w) and not wt[40:].any() and not wt[:, 72:].any()
    fwd = pack_linear(w, torch.zeros(40))[0]
    assert torch.equal(fwd[:72, :40], wt[:40, :72].t())
    conv = torch.randn(24, 3, 8, 8, generator=gen)
    f, (b, bias, cop, bn) = pack_patch_embedding(conv)[0], pack_patch_embedding_transposed(conv)
    assert b.shape == (32, 256) and cop == 256 and not bias.any()
    assert torch.equal(b[:24], f[:, :24].t()) and not b[24:].any()


# ---- the loss heads -------------------------------------------------------------------------------------------------------------
def _embeddings(n=5, d=32, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=gen) * 3, torch.randn(n, d, generator=gen) * 3, torch.randn(d, generator=gen)


def test_loss_heads_vs_fp64_formulas():
    """Values and gradients.  fp32 compositions of a few hundred operations on O(1) values against fp64: 64 ulp of fp32
    relative to the max-norm."""
    from rick_amd import clipguide
    e_t, e_s, direction = _embeddings()
    bound = 64 * 2.0 ** -24
    for mine, ref in ((lambda t: clipguide.directional_loss(t, e_s, direction), lambda t: R.directional_loss_f64(t, e_s, direction)),
                      (lambda t: clipguide.within_loss(t, e_s), lambda t: R.within_loss_f64(t, e_s))):
        t32, t64 = e_t.clone().requires_grad_(), e_t.double().requires_grad_()
        a, b = mine(t32), ref(t64)
        assert a.dtype == torch.float32 and a.dim() == 0
        assert abs(float(a.detach()) - float(b.detach())) <= bound * abs(float(b.detach())) and float(b.detach()) > 0
        (ga,), (gb,) = torch.autograd.grad(a, t32), torch.autograd.grad(b, t64)
        assert float(gb.abs().max()) > 0 and max_rel_err(ga, gb) <= bound


def test_loss_heads_at_their_minimum():
    from rick_amd import clipguide
    e_t, e_s, direction = _embeddings()
    assert abs(float(clipguide.within_loss(e_s, e_s))) <= 2.0 ** -22                    # identical sets: 0 (cos = 1 to rounding)
    assert abs(float(clipguide.within_loss(e_s * 2.5, e_s))) <= 2.0 ** -22              # the scale of an embedding does not matter


def test_directional_loss_of_a_step_along_the_direction_is_zero_to_rounding():
    """e_t = e_s + c direction with both on the unit sphere (the chord along the direction, c > 0), where normalisation is the
    identity: the loss is 0 to rounding, against the opposite direction it is 2, and the embeddings' scales do not matter."""
    from rick_amd import clipguide
    gen = torch.Generator().manual_seed(3)
    direction = torch.nn.functional.normalize(torch.randn(32, generator=gen), dim=0)
    e_s = torch.nn.functional.normalize(torch.randn(6, 32, generator=gen), dim=1)
    e_s = torch.nn.functional.normalize(e_s - (e_s @ direction)[:, None] * direction - 0.5 * direction, dim=1)   # s . direction < 0
    c = -2 * (e_s @ direction)
    e_t = e_s + c[:, None] * direction                        # unit again: the chord of the sphere along the direction
    assert float((e_t.norm(dim=1) - 1).abs().max()) <= 2.0 ** -21
    assert float(c.min()) > 0.5
    assert abs(float(clipguide.directional_loss(e_t, e_s, direction))) <= 2.0 ** -20
    assert abs(float(clipguide.directional_loss(e_t * 4, e_s * 0.3, direction * 7))) <= 2.0 ** -20
    assert abs(float(clipguide.directional_loss(e_t, e_s, -direction)) - 2) <= 2.0 ** -20


def test_domain_direction_and_guide():
    from rick_amd import clipguide
    net = _net_a()
    src, tgt = clip_images(4, 32, seed=1), clip_images(5, 32, seed=2)
    d = clipguide.domain_direction(net, src, tgt)
    assert d.shape == (32,) and d.dtype == torch.float32 and not d.requires_grad
    assert max_rel_err(d, R.domain_direction_f64(net(src), net(tgt))) <= 64 * 2.0 ** -24
    guide = clipguide.ClipGuide(net, d)
    x = clip_images(3, 32, seed=3).requires_grad_()
    terms = guide.terms(x, clip_images(3, 32, seed=4))
    assert set(terms) == {'clip_dir', 'clip_within'}
    (g,) = torch.autograd.grad(terms['clip_dir'] + terms['clip_within'], x)
    assert torch.isfinite(g).all() and g.any()
    assert set(guide.terms(x, clip_images(3, 32, seed=4), within=False)) == {'clip_dir'}
    with pytest.raises(ValueError, match='direction'):
        clipguide.ClipGuide(net, torch.zeros(31))
    with pytest.raises(ValueError, match='at least 2'):
        clipguide.within_loss(torch.randn(1, 32), torch.randn(1, 32))
    with pytest.raises(ValueError, match='one shape'):
        clipguide.directional_loss(torch.randn(2, 32), torch.randn(3, 32), d)
    with pytest.raises(ValueError, match='direction'):
        clipguide.directional_loss(torch.randn(2, 32), torch.randn(2, 32), torch.randn(2, 32))


# ---- the trainer's validation -----------------------------------------------------------------------------------------------
def test_train_config_fields_and_validation():
    from rick_amd.clipguide import ClipGuide
    from rick_amd.train import RickTrainer, TrainConfig
    cfg = TrainConfig()
    assert (cfg.clip_dir_weight, cfg.clip_within_weight, cfg.clip_batch) == (0.0, 0.0, 4)
    g = torch.nn.Linear(2, 2)
    guide = ClipGuide(_net_a(), torch.ones(32))

    def build(**kw):
        args = {k: kw.pop(k) for k in ('g_source', 'clip') if k in kw}
        return RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, **kw), g, g, g, g, **args)
    for kw in (dict(clip_dir_weight=-1.0), dict(clip_within_weight=float('nan')), dict(clip_dir_weight=float('inf'))):
        with pytest.raises(ValueError, match='clip_dir_weight and clip_within_weight must be finite'):
            build(**kw)
    src = torch.nn.Linear(2, 2)
    for kw in (dict(clip_dir_weight=1.0), dict(clip_within_weight=1.0, g_source=src), dict(clip_dir_weight=1.0, clip=guide)):
        with pytest.raises(ValueError, match='need the frozen source generator and the CLIP guide'):
            build(**kw)
    with pytest.raises(ValueError, match='clip_batch'):
        build(clip_within_weight=1.0, clip_batch=1, g_source=src, clip=guide)
    with pytest.raises(ValueError, match='clip_batch'):
        build(clip_dir_weight=1.0, clip_batch=0, g_source=src, clip=guide)
