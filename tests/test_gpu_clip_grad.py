"""GPU: the data-gradient kernels of the CLIP image tower (rick_amd/csrc/clip.hip) through the C ABI against the hand-written
fp64 adjoints of tests/clip_grad_f64.py, ``ClipImageFeatures.encode`` against torch fp64 autograd of the independent fp64
restatement (tests/clip_f64.py), the CLIP-space losses end to end and the trainer's CLIP terms.  Every kernel test puts a
sentinel guard row behind its output.

Tolerances: the rule of tests/test_gpu_clip.py.  The base figure of a comparison is the error of the fp32 torch CPU autograd
composition against the same fp64 reference on the same inputs (max error over the reference's max-norm, measured once on the
CPU with `python -m tests.clip_grad_f64` and written down below next to its shape); the device bound is that figure x 4.  No
element is excluded, and every gradient test asserts that the reference is not zero."""
import pytest
import torch

from tests import clip_grad_f64 as R
from tests.clip_f64 import SmoothG, embed_f64, max_rel_err, synthetic_clip_state_dict
from tests.test_gpu_clip import CONFIGS, _Gemm, network, network_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0
FACTOR = 4

QGELU_BWD_CPU_BASE = 4.590e-07                                   # quickgelu_bwd_inputs(): 51 x 192, u ~ 3 N(0, 1)
LN_BWD_CPU_BASE = {(51, 64): 1.368e-07, (5, 36): 1.097e-07, (3, 1024): 1.101e-07, (51, 768): 1.273e-07}
LN_BWD_STRIDED_CPU_BASE = 1.161e-07                              # every 17th row of 51 x 64
LN_BWD_OFFSET_CPU_BASE = 1.960e-06                               # 51 x 768, mean 100, standard deviation 1
# attention_bwd_inputs(T, d, heads, qscale): (dq, dk, dv) as is and with queries x 30
ATT_BWD_CPU_BASE = {(17, 16, 4): ((2.312e-07, 2.416e-07, 2.018e-07), (1.574e-06, 1.912e-06, 1.138e-06)),
                    (50, 64, 2): ((3.645e-07, 4.154e-07, 3.518e-07), (3.710e-06, 4.170e-06, 1.566e-06)),
                    (82, 32, 2): ((4.173e-07, 4.107e-07, 4.788e-07), (3.595e-06, 5.426e-06, 1.326e-06)),
                    (257, 64, 1): ((8.105e-07, 6.132e-07, 5.853e-07), (7.621e-06, 8.502e-06, 3.795e-06))}
TOKENS_BWD_CPU_BASE = 1.536e-07                                  # tokens_bwd_inputs(): 3 x 17 x 64
INPUT_BWD_CPU_BASE = {(256, 256): 2.295e-05, (64, 64): 6.303e-06, (100, 317): 2.103e-05}      # input_bwd_inputs(224) -> (H, W)
# d sum(emb * r) / dx: ClipImageFeatures.encode on CPU tensors (torch autograd, fp32) against autograd of embed_f64, on
# network_inputs(cfg, size)[:n] and network_upstream(n, dim).  B from 256^2: 23 % of the gradient are exact zeros (the
# downscale skips pixels)
NET_GRAD_CPU_BASE = {('A', 32, 3): 3.593e-07, ('A', 64, 3): 4.637e-07, ('B', 256, 3): 1.855e-05, ('A', 32, 8): 5.071e-07,
                     ('A', 64, 8): 9.272e-07, ('B', 256, 8): 1.855e-05}


def _lib():
    from rick_amd import _lib
    return _lib


def _check(what, got, ref, base):
    assert float(ref.abs().max()) > 0
    err = max_rel_err(got, ref)
    print(f'{what}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert torch.isfinite(got).all()
    assert err <= FACTOR * base, what


def _guarded(rows, cols):
    return torch.full((rows + 1, cols), SENTINEL, device=DEV)


# ---- QuickGELU ------------------------------------------------------------------------------------------------------------
def test_quickgelu_kernel_equals_the_gemm_epilogue():
    L = _lib()
    gemm = _Gemm('51x64x192')
    u, want = gemm(0, None), gemm(1, None)
    out = _guarded(51, 192)
    L.check(L.lib.rick_clip_quickgelu_f32(u.data_ptr(), out.data_ptr(), u.numel(), L.stream_ptr()), 'rick_clip_quickgelu_f32')
    assert torch.all(out[51] == SENTINEL)
    assert torch.equal(out[:51], want)


def test_quickgelu_bwd_vs_fp64():
    L = _lib()
    u, g = R.quickgelu_bwd_inputs()
    ud, out = u.to(DEV), _guarded(51, 192)
    L.check(L.lib.rick_clip_quickgelu_bwd_f32(ud.data_ptr(), g.to(DEV).data_ptr(), out.data_ptr(), u.numel(), L.stream_ptr()),
            'rick_clip_quickgelu_bwd_f32')
    assert torch.all(out[51] == SENTINEL)
    _check('rick_clip_quickgelu_bwd_f32 51 x 192', out[:51].cpu(), R.quickgelu_grad_f64(u, g), QGELU_BWD_CPU_BASE)
    inplace = _guarded(51, 192)
    inplace[:51] = g.to(DEV)
    L.check(L.lib.rick_clip_quickgelu_bwd_f32(ud.data_ptr(), inplace.data_ptr(), inplace.data_ptr(), u.numel(), L.stream_ptr()),
            'rick_clip_quickgelu_bwd_f32')
    assert torch.equal(inplace, out)


# ---- LayerNorm backward ---------------------------------------------------------------------------------------------------
def run_layernorm_bwd(x, w, g, add=None, rows=None, ld=None, addend=None):
    """add: None, 'separate' or 'inplace', the addend being zeros unless given; rows / ld: R rows at the stride ld in x and
    out (g compact).  Returns the whole output buffer without the guard row."""
    L = _lib()
    C = w.numel()
    R_ = rows if rows is not None else x.shape[0]
    ld = ld or C
    total = x.numel() // C
    xd, wd, gd = x.to(DEV).contiguous(), w.to(DEV), g.to(DEV).contiguous()
    out = _guarded(total, C)
    addp = None
    ad = torch.zeros(total, C, device=DEV) if addend is None else addend.to(DEV).contiguous()
    if add == 'separate':
        addp = ad.data_ptr()
    elif add == 'inplace':
        out[:total] = ad
        addp = out.data_ptr()
    L.check(L.lib.rick_clip_layernorm_bwd_f32(xd.data_ptr(), ld, wd.data_ptr(), gd.data_ptr(), C, addp, out.data_ptr(), ld, R_, C, 1e-5,
                                              L.stream_ptr()), 'rick_clip_layernorm_bwd_f32')
    assert torch.all(out[total] == SENTINEL)
    return out[:total].cpu()


@pytest.mark.parametrize('R_,C', list(LN_BWD_CPU_BASE))
def test_layernorm_bwd_vs_fp64(R_, C):
    x, w, g = R.layernorm_bwd_inputs(R_, C)
    got = run_layernorm_bwd(x, w, g)
    _check(f'rick_clip_layernorm_bwd_f32 {R_} x {C}', got, R.layernorm_grad_f64(x, w, g), LN_BWD_CPU_BASE[(R_, C)])
    assert torch.equal(run_layernorm_bwd(x, w, g), got)                       # run to run
    # add = NULL, a separate buffer of zeros and zeros in place: the same bits in all three
    assert torch.equal(run_layernorm_bwd(x, w, g, 'separate'), got) and torch.equal(run_layernorm_bwd(x, w, g, 'inplace'), got)
    # a residual gradient as the addend: in place as from a separate buffer, and dx + add to one fp32 rounding of the sum
    sep = run_layernorm_bwd(x, w, g, 'separate', addend=x)
    assert torch.equal(run_layernorm_bwd(x, w, g, 'inplace', addend=x), sep)
    assert float((sep.double() - (got.double() + x.double())).abs().max()) <= 2.0 ** -23 * float((got.abs() + x.abs()).max())


def test_layernorm_bwd_writes_rows_with_a_stride():
    x, w, g = R.layernorm_bwd_inputs(51, 64)                                  # 3 images of 17 tokens: token 0 of every image
    got = run_layernorm_bwd(x, w, g[::17], rows=3, ld=17 * 64)
    _check('rick_clip_layernorm_bwd_f32 every 17th row', got[::17], R.layernorm_grad_f64(x[::17], w, g[::17]), LN_BWD_STRIDED_CPU_BASE)
    keep = torch.ones(51, dtype=torch.bool)
    keep[::17] = False
    assert torch.all(got[keep] == SENTINEL)                                   # the other rows of out are untouched
    assert torch.equal(got[::17], run_layernorm_bwd(x[::17].contiguous(), w, g[::17]))


def test_layernorm_bwd_with_a_large_mean():
    x, w, g = R.layernorm_bwd_inputs(51, 768, offset=True)
    _check('rick_clip_layernorm_bwd_f32 mean 100, std 1', run_layernorm_bwd(x, w, g), R.layernorm_grad_f64(x, w, g), LN_BWD_OFFSET_CPU_BASE)


def test_layernorm_bwd_and_tokens_bwd_reject_what_they_do_not_support():
    L = _lib()
    t = torch.zeros(1 << 14, device=DEV)
    p, s = t.data_ptr(), L.stream_ptr()
    assert L.lib.rick_clip_layernorm_bwd_f32(p, 64, p, p, 64, None, p, 64, 4, 64, 1e-5, s) == 0
    for R_, C, ld in ((4, 62, 64), (4, 2052, 2052), (4, 64, 32), (4, 64, 66), (-1, 64, 64)):
        assert L.lib.rick_clip_layernorm_bwd_f32(p, ld, p, p, 64 if C == 64 else C, None, p, 64 if C == 64 else C, R_, C, 1e-5, s) == 22
    assert L.lib.rick_clip_layernorm_bwd_f32(p, 64, p, p, 32, None, p, 64, 4, 64, 1e-5, s) == 22
    assert L.lib.rick_clip_layernorm_bwd_f32(p, 64, p, p, 64, None, p, 66, 4, 64, 1e-5, s) == 22
    assert L.lib.rick_clip_layernorm_bwd_f32(None, 64, p, p, 64, None, p, 64, 4, 64, 1e-5, s) == 22
    assert L.lib.rick_clip_tokens_bwd_f32(p, p, p, p, p, 2, 258, 16, 1e-5, s) == 22
    assert L.lib.rick_clip_tokens_bwd_f32(p, p, p, p, p, 2, 5, 18, 1e-5, s) == 22
    torch.cuda.synchronize()


def test_tokens_bwd_vs_fp64():
    L = _lib()
    patches, pos, w, g = R.tokens_bwd_inputs()
    N, T, C = g.shape
    out = _guarded(N * (T - 1), C)
    dev = [v.to(DEV) for v in (patches, pos, w, g)]
    L.check(L.lib.rick_clip_tokens_bwd_f32(*(v.data_ptr() for v in dev), out.data_ptr(), N, T, C, 1e-5, L.stream_ptr()), 'rick_clip_tokens_bwd_f32')
    assert torch.all(out[N * (T - 1)] == SENTINEL)
    got = out[:N * (T - 1)].view(N, T - 1, C).cpu()
    _check('rick_clip_tokens_bwd_f32 3 x 17 x 64', got, R.tokens_grad_f64(patches, pos, w, g), TOKENS_BWD_CPU_BASE)


# ---- attention backward ---------------------------------------------------------------------------------------------------
def run_attention_bwd(qkv, go, d, heads):
    L = _lib()
    n, T, _ = qkv.shape
    qd, gd = qkv.to(DEV).contiguous(), go.to(DEV).contiguous()
    out = _guarded(n * T, 3 * heads * d)
    stats = torch.full((n * heads * T + 1, 3), SENTINEL, device=DEV)
    L.check(L.lib.rick_clip_attention_bwd_f32(qd.data_ptr(), gd.data_ptr(), stats.data_ptr(), out.data_ptr(), n, T, heads, d, L.stream_ptr()),
            'rick_clip_attention_bwd_f32')
    assert torch.all(out[n * T] == SENTINEL) and torch.all(stats[n * heads * T] == SENTINEL)
    return out[:n * T].view(n, T, 3 * heads * d).cpu()


@pytest.mark.parametrize('T,d,heads', list(ATT_BWD_CPU_BASE))
def test_attention_bwd_vs_fp64(T, d, heads):
    wd = heads * d
    for i, qscale in enumerate((1.0, 30.0)):
        qkv, go = R.attention_bwd_inputs(T, d, heads, qscale)
        got, ref = run_attention_bwd(qkv, go, d, heads), R.attention_grad_f64(qkv, go, d, heads)
        for j, name in enumerate(('dq', 'dk', 'dv')):
            _check(f'rick_clip_attention_bwd_f32 T={T} d={d} heads={heads} q x {qscale:g} {name}', got[..., j * wd:(j + 1) * wd],
                   ref[..., j * wd:(j + 1) * wd], ATT_BWD_CPU_BASE[(T, d, heads)][i][j])
        assert torch.equal(run_attention_bwd(qkv, go, d, heads), got)         # run to run


@pytest.mark.parametrize('T,d,heads', [(17, 16, 4), (257, 64, 1)])
def test_attention_bwd_of_an_image_does_not_depend_on_the_batch(T, d, heads):
    qkv, go = R.attention_bwd_inputs(T, d, heads)
    full = run_attention_bwd(qkv, go, d, heads)
    assert torch.equal(run_attention_bwd(qkv[1:2], go[1:2], d, heads), full[1:2])              # alone
    assert torch.equal(run_attention_bwd(qkv.flip(0), go.flip(0), d, heads)[2], full[0])       # last in a flipped batch
    gen = torch.Generator().manual_seed(9)
    oq, og = torch.randn(qkv.shape, generator=gen), torch.randn(go.shape, generator=gen)
    oq[1], og[1] = qkv[1], go[1]
    assert torch.equal(run_attention_bwd(oq, og, d, heads)[1], full[1])       # beside different images


def test_attention_bwd_rejects_what_it_does_not_support():
    L = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    p, s = t.data_ptr(), L.stream_ptr()
    assert L.lib.rick_clip_attention_bwd_f32(p, p, p, p, 1, 5, 2, 16, s) == 0
    for T, heads, d in ((258, 1, 16), (0, 1, 16), (5, 2, 48), (5, 2, 128), (5, 0, 16)):
        assert L.lib.rick_clip_attention_bwd_f32(p, p, p, p, 1, T, heads, d, s) == 22
    assert L.lib.rick_clip_attention_bwd_f32(None, p, p, p, 1, 5, 2, 16, s) == 22
    torch.cuda.synchronize()


# ---- input adjoint --------------------------------------------------------------------------------------------------------
def run_input_bwd(g, H, W, P):
    """g [N, 3, S, S] -> [N, 3, H, W] through the patch-row layout."""
    L = _lib()
    N, _, S, _ = g.shape
    rows = R.patch_rows(g, P).to(DEV)
    out = torch.full((N + 1, 3, H, W), SENTINEL, device=DEV)                   # one guard image behind the output
    L.check(L.lib.rick_clip_input_bwd_f32(rows.data_ptr(), out.data_ptr(), N, H, W, S, P, L.stream_ptr()), 'rick_clip_input_bwd_f32')
    assert torch.all(out[N] == SENTINEL)
    return out[:N].cpu()


@pytest.mark.parametrize('hw', list(INPUT_BWD_CPU_BASE))
def test_input_bwd_vs_fp64(hw):
    g = R.input_bwd_inputs(224)                                               # G = 7, P = 32
    got = run_input_bwd(g, *hw, 32)
    _check(f'rick_clip_input_bwd_f32 224 -> {hw}', got, R.input_bwd_autograd_f64(g, *hw), INPUT_BWD_CPU_BASE[hw])
    assert torch.equal(run_input_bwd(g, *hw, 32), got)                        # run to run


def test_input_bwd_at_the_output_size_is_the_affine_alone():
    g = R.input_bwd_inputs(32)
    std = torch.tensor((0.26862954, 0.26130258, 0.27577711)).view(1, 3, 1, 1)
    for P in (8, 32):
        assert torch.equal(run_input_bwd(g, 32, 32, P), g * 0.5 / std)


def test_input_bwd_rejects_what_it_does_not_support():
    L = _lib()
    t = torch.zeros(1 << 14, device=DEV)
    p, s = t.data_ptr(), L.stream_ptr()
    assert L.lib.rick_clip_input_bwd_f32(p, p, 1, 8, 8, 16, 8, s) == 0
    for H, W, S, P in ((0, 8, 16, 8), (8, 8, 16, 5), (8, 8, 16, 0), (8, 8, 0, 8)):
        assert L.lib.rick_clip_input_bwd_f32(p, p, 1, H, W, S, P, s) == 22
    torch.cuda.synchronize()


# ---- whole network --------------------------------------------------------------------------------------------------------
_GRAD_REF = {}


def network_grad_reference(name, size, n):
    """(x, r, d sum(embed_f64(x) * r) / dx), computed once per case."""
    if (name, size, n) not in _GRAD_REF:
        cfg, heads = CONFIGS[name]
        x, r = network_inputs(name, size)[:n], R.network_upstream(n, cfg['dim'])
        x64 = x.double().requires_grad_()
        (embed_f64(synthetic_clip_state_dict(cfg, 11), x64, heads) * r.double()).sum().backward()
        _GRAD_REF[(name, size, n)] = (x, r, x64.grad)
    return _GRAD_REF[(name, size, n)]


def _grad(net, x, r):
    xd = x.to(DEV).requires_grad_()
    emb = net.encode(xd)
    (g,) = torch.autograd.grad((emb * r.to(DEV)).sum(), xd)
    return emb.detach(), g


@pytest.mark.parametrize('name,size,n', list(NET_GRAD_CPU_BASE))
def test_encode_value_and_gradient_vs_fp64(name, size, n):
    net = network(name)
    x, r, ref = network_grad_reference(name, size, n)
    before = net(x.to(DEV))
    emb, g = _grad(net, x, r)
    assert torch.equal(emb, before)                                           # the value: bit for bit
    assert torch.equal(net(x.to(DEV)), before)                                # __call__ after prepare_grad: unchanged
    assert g.dtype == torch.float32 and g.shape == x.shape and g.device.type == 'cuda'
    _check(f'CLIP {name} from {size}^2, n={n}: d sum(emb r) / dx', g.cpu(), ref, NET_GRAD_CPU_BASE[(name, size, n)])
    assert torch.equal(_grad(net, x, r)[1], g)                                # run to run
    assert not net.encode(x.to(DEV)).requires_grad                            # without grad it is __call__


@pytest.mark.parametrize('name,size', [('A', 64), ('B', 256)])
def test_encode_layouts_and_batches_give_the_same_bits(name, size):
    x, r, _ = network_grad_reference(name, size, 8)
    emb, g = _grad(network(name), x, r)
    for layout in ('openai', 'openai-visual'):
        e2, g2 = _grad(network(name, layout), x, r)
        assert torch.equal(e2, emb) and torch.equal(g2, g)
    assert torch.equal(_grad(network(name), x[2:3], r[2:3])[1], g[2:3])       # alone
    assert torch.equal(_grad(network(name), x.flip(0), r.flip(0))[1].flip(0), g)


def test_encode_refuses_what_it_cannot_do():
    net = network('A')
    x, r, _ = network_grad_reference('A', 32, 8)
    xd = x.to(DEV).requires_grad_()
    first = net.encode(xd)
    net.encode(xd).sum().backward()                                           # a later differentiable call
    with pytest.raises(RuntimeError, match='overwritten by a later differentiable call'):
        first.sum().backward()
    with pytest.raises(RuntimeError, match='first order only'):
        torch.autograd.grad(net.encode(xd).sum(), xd, create_graph=True)
    with pytest.raises(ValueError, match='grad_batch'):
        net.encode(torch.cat([xd, xd[:1]]))
    with pytest.raises(ValueError, match='grad_batch'):
        net.prepare_grad(grad_batch=26)                                       # above the plan's batch of 25


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _guide_inputs():
    gen = torch.Generator().manual_seed(21)
    z = torch.randn(4, 512, generator=gen)
    src = network_inputs('A', 32)[:4]
    direction = torch.nn.functional.normalize(torch.randn(32, generator=gen), dim=0)
    return z, src, direction


def _composed(net_cpu, img, src, direction, dtype):
    """directional + within loss by torch composition on the CPU in `dtype`: the network is embed_f64 (fp64) or the fp32 torch
    composition (ClipImageFeatures on CPU tensors)."""
    cfg, heads = CONFIGS['A']
    if dtype == torch.float64:
        sd = synthetic_clip_state_dict(cfg, 11)
        e_t, e_s = embed_f64(sd, img.double(), heads), embed_f64(sd, src, heads)
        return R.directional_loss_f64(e_t, e_s, direction), R.within_loss_f64(e_t, e_s)
    from rick_amd import clipguide
    e_t, e_s = net_cpu.encode(img), net_cpu(src)
    return clipguide.directional_loss(e_t, e_s, direction), clipguide.within_loss(e_t, e_s)


def test_generator_gradient_through_the_clip_losses_vs_fp64():
    """SmoothG(32) -> encode -> directional + within loss: the gradient with respect to the latents (the generator's input; its
    only parameter does not reach the image) on the device against the fp64 CPU composition, by the rule above."""
    from rick_amd import clipguide
    from rick_amd.clip import ClipImageFeatures
    cfg, heads = CONFIGS['A']
    net, net_cpu = network('A'), ClipImageFeatures.load(synthetic_clip_state_dict(cfg, 11), device='cpu', heads=heads)
    z, src, direction = _guide_inputs()
    grads = {}
    for key, dtype in (('f64', torch.float64), ('f32', torch.float32)):
        g, zz = SmoothG(32).to(dtype), z.to(dtype).requires_grad_()
        grads[key] = torch.autograd.grad(sum(_composed(net_cpu, g([zz])[0], src, direction, dtype)), zz)[0]
    g, zd = SmoothG(32).to(DEV), z.to(DEV).requires_grad_()
    e_t, e_s = net.encode(g([zd])[0]), net(src.to(DEV))
    loss = clipguide.directional_loss(e_t, e_s, direction.to(DEV)) + clipguide.within_loss(e_t, e_s)
    (got,) = torch.autograd.grad(loss, zd)
    base = max_rel_err(grads['f32'], grads['f64'])
    _check('SmoothG -> encode -> directional + within: d loss / dz', got.cpu(), grads['f64'], base)


# ---- trainer --------------------------------------------------------------------------------------------------------------
def _build():
    from rick_amd.models import Discriminator, Generator
    torch.manual_seed(11)
    g0, d0 = Generator(32, 512, 2), Discriminator(32)

    def make(perturb=0.0):
        g, d = Generator(32, 512, 2), Discriminator(32)
        g.load_state_dict(g0.state_dict())
        d.load_state_dict(d0.state_dict())
        if perturb:
            gen = torch.Generator().manual_seed(1)
            with torch.no_grad():
                for n, p in g.named_parameters():
                    if n.startswith('convs.'):
                        p.add_(perturb * p.abs().mean() * torch.randn(p.shape, generator=gen))
        return g.to(DEV), d.to(DEV)
    return make


def _trainer(make, weights, guide=True):
    from rick_amd.clipguide import ClipGuide
    from rick_amd.train import RickTrainer, TrainConfig
    g, d = make(perturb=0.3)
    g_ema, d_ema = make()
    src = make()[0]
    cfg = TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, clip_batch=2, clip_dir_weight=weights[0], clip_within_weight=weights[1])
    kw = dict(clip=ClipGuide(network('A'), _guide_inputs()[2])) if guide else {}
    return RickTrainer(cfg, g, d, g_ema, d_ema, g_source=src, **kw), src


def _fixed(g):
    gen = torch.Generator(DEV).manual_seed(7)
    maps = [torch.randn(n.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(2 + i)) for i, n in enumerate(g.make_noise())]
    return dict(noise=[torch.randn(2, 512, device=DEV, generator=gen)], g_noise=maps)


def test_trainer_clip_terms_vs_fp64_and_weight_zero():
    from rick_amd.clip import ClipImageFeatures
    make = _build()
    tr, src = _trainer(make, (1.5, 0.7))
    fixed = _fixed(tr.g)
    clip_noise = torch.randn(2, 512, device=DEV, generator=torch.Generator(DEV).manual_seed(8))
    with torch.no_grad():
        img_t, img_s = tr.g([clip_noise], noise=fixed['g_noise'])[0].cpu(), src([clip_noise], noise=fixed['g_noise'])[0].cpu()
    tr.g_step(**fixed, clip_noise=clip_noise)
    cfg, heads = CONFIGS['A']
    net_cpu = ClipImageFeatures.load(synthetic_clip_state_dict(cfg, 11), device='cpu', heads=heads)
    direction = _guide_inputs()[2]
    with torch.no_grad():
        ref = torch.stack(_composed(net_cpu, img_t, img_s, direction, torch.float64))
        cpu = torch.stack(_composed(net_cpu, img_t, img_s, direction, torch.float32))
    got = torch.stack([tr.losses['clip_dir'], tr.losses['clip_within']]).cpu()
    print(f'trainer clip_dir, clip_within: {got.tolist()}, fp64 {ref.tolist()}, fp32 CPU {cpu.tolist()}')
    _check('trainer (clip_dir, clip_within)', got, ref, max_rel_err(cpu, ref))
    # the step with the terms moves G differently from the step without them; weights 0 = a trainer built without clip=
    after_on = {n: p.detach().clone() for n, p in tr.g.named_parameters()}
    results = []
    for guide in (True, False):
        tr0, _ = _trainer(make, (0.0, 0.0), guide)
        tr0.g_step(**_fixed(tr0.g), clip_noise=clip_noise)
        assert 'clip_dir' not in tr0.losses and 'clip_within' not in tr0.losses
        results.append({n: p.detach().clone() for n, p in tr0.g.named_parameters()})
    assert all(torch.equal(results[0][n], results[1][n]) for n in results[0])
    assert any(not torch.equal(after_on[n], results[0][n]) for n in after_on)
    assert all(torch.isfinite(p).all() for p in after_on.values())


def test_call_is_unchanged_by_prepare_grad():
    from rick_amd.clip import ClipImageFeatures
    cfg, heads = CONFIGS['A']
    net = ClipImageFeatures.load(synthetic_clip_state_dict(cfg, 11), device=DEV, batch=5, heads=heads)
    x = network_inputs('A', 64)[:7].to(DEV)
    before = net(x)
    assert net.prepare_grad(grad_batch=3) is net
    assert torch.equal(net(x), before)
    assert torch.equal(net.encode(x[:3].clone().requires_grad_()), before[:3])
