"""rick_gram_f32 / rick_rowmix_f32 and the distance-consistency loss on them (rick_amd/cdc.py, rick_amd/csrc/gram.hip) against
fp64, and the trainer's G step with the term.

Every bound follows DESIGN.md section 7: four times the error that the plain fp32 torch composition of the same quantity makes
against the same fp64 reference on the same inputs, measured here per shape (never a constant).  The figures each test prints
(run with -s) are the ones quoted in DESIGN.md section 7."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (B, n): one element; fewer than a float4; a partial block, rows unaligned; two slices with unaligned rows; two full slices,
# aligned; 17 slices, n % 4 == 3; past 4096 * 1024 elements, where the slices grow to 8192 (both load paths)
GRAM_SHAPES = [(1, 1), (2, 3), (3, 255), (4, 4097), (8, 8192), (5, 67015), (2, 4096 * 1024 + 4101), (2, 4096 * 1024 + 4104)]
_cache = {}


def _case(shape):
    """x fp32 [B, ...] on the CPU (N(0, 1) + 1: cosines near 1, as behind a LeakyReLU), its rows in memory order as fp64, and the
    fp64 Gram matrix — computed once per shape and shared."""
    if shape not in _cache:
        g = torch.Generator().manual_seed(99 if isinstance(shape, str) else sum(shape))
        if shape == 'channels_last':
            x = (torch.randn(4, 24, 9, 7, generator=g) + 1.0).contiguous(memory_format=torch.channels_last)
            rows = x.permute(0, 2, 3, 1).reshape(4, -1)
        else:
            x = torch.randn(*shape, generator=g) + 1.0
            rows = x
        r64 = rows.double()
        _cache[shape] = (x, rows, r64, r64 @ r64.t())
    return _cache[shape]


def _gram_err(G, ref):
    d = torch.diagonal(ref).sqrt()
    return float(((G.double().cpu() - ref).abs() / (d[:, None] * d[None, :])).max())


def _ids(s):
    return s if isinstance(s, str) else f'{s[0]}x{s[1]}'


@pytest.mark.parametrize('shape', GRAM_SHAPES + ['channels_last'], ids=_ids)
def test_gram_vs_fp64(shape):
    from rick_amd import cdc
    x, rows, _, ref = _case(shape)
    base = _gram_err(rows @ rows.t(), ref)                     # the fp32 torch composition on the CPU
    xd = x.to(DEV)
    G = cdc.gram(xd)
    err = _gram_err(G, ref)
    print(f'gram {_ids(shape)}: device {err:.3e}  fp32 composition {base:.3e}  bound {4 * base:.3e}')
    assert G.dtype == torch.float64 and G.shape == (x.shape[0],) * 2
    assert torch.equal(G, G.t())                               # exactly symmetric
    assert torch.equal(G, cdc.gram(xd))                        # run to run
    assert err <= 4 * base


@pytest.mark.parametrize('shape', [(4, 4097), (5, 67015), (8, 8192), 'channels_last'], ids=_ids)
def test_gram_entry_depends_on_its_two_rows_alone(shape):
    from rick_amd import cdc
    x = _case(shape)[0].to(DEV)
    G = cdc.gram(x)
    sub = x[[1, 3]].contiguous(memory_format=torch.channels_last if shape == 'channels_last' else torch.contiguous_format)
    assert torch.equal(cdc.gram(sub), G[[1, 3]][:, [1, 3]])
    assert torch.equal(cdc.gram(x[3:4]), G[3:4, 3:4])          # a view into the batch: another address, the same sums


@pytest.mark.parametrize('shape', GRAM_SHAPES + ['channels_last'], ids=_ids)
def test_rowmix_vs_fp64(shape):
    from rick_amd import cdc
    _, rows, r64, _ = _case(shape)
    B = rows.shape[0]
    xd = rows.to(DEV)
    # A comes from a preceding device op and is never copied to the host before the launch
    Ad = torch.randn(B, B, device=DEV, generator=torch.Generator(DEV).manual_seed(B))
    Ad = Ad + Ad.t()
    y = cdc.rowmix(Ad, xd)
    A = Ad.cpu()
    ref = A.double() @ r64
    scale = ref.abs().max()
    base = float(((A @ rows).double() - ref).abs().max() / scale)
    err = float((y.double().cpu() - ref).abs().max() / scale)
    print(f'rowmix {_ids(shape)}: device {err:.3e}  fp32 composition {base:.3e}  bound {4 * base:.3e}')
    assert err <= 4 * base
    assert torch.equal(cdc.rowmix(torch.eye(B, device=DEV), xd), xd)
    Az = Ad.clone()
    Az[B - 1] = 0
    yz = cdc.rowmix(Az, xd)
    assert not yz[B - 1].any() and torch.equal(yz[:B - 1], y[:B - 1])


def test_gram_backward_is_rowmix_in_the_layout_of_x():
    from rick_amd import cdc
    x, rows, r64, _ = _case('channels_last')
    xd = x.to(DEV).requires_grad_(True)
    w = torch.randn(4, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    (g,) = torch.autograd.grad((cdc.gram(xd) * w.to(DEV)).sum(), xd)
    assert g.stride() == xd.stride() and g.shape == xd.shape
    A = (w + w.t()).float()
    ref = (A.double() @ r64).view(4, 9, 7, 24).permute(0, 3, 1, 2)
    base = float(((A @ rows).view(4, 9, 7, 24).permute(0, 3, 1, 2).double() - ref).abs().max() / ref.abs().max())
    err = float((g.double().cpu() - ref).abs().max() / ref.abs().max())
    assert err <= 4 * base
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(cdc.gram(xd).sum(), xd, create_graph=True)


# ---- loss and gradient with respect to the features ---------------------------------------------------------------------------
FEAT_SHAPES = [(8, 4, 4), (16, 8, 8), (5, 7, 9), (3, 33, 31)]


def _loss_fp32(feats_t, feats_s, layers):
    """The loss as a plain fp32 torch composition (Gram matrix by matmul, everything in fp32): the base of the fourfold rule."""
    def cosines(feats):
        rows = []
        for i, l in enumerate(layers):
            X = feats[l].flatten(1)
            G = X @ X.t()
            n = torch.diagonal(G).sqrt().clamp_min(1e-8)
            c = G[i] / (n[i] * n)
            rows.append(torch.cat([c[:i], c[i + 1:]]))
        return torch.stack(rows)
    with torch.no_grad():
        lps = torch.log_softmax(cosines(feats_s), 1)
    return (lps.exp() * (lps - torch.log_softmax(cosines(feats_t), 1))).mean()


@pytest.mark.parametrize('layers', [[0, 1, 2, 3], [2, 0, 2, 2]], ids=['distinct', 'repeated'])
def test_loss_and_feature_gradients_vs_fp64(layers):
    from rick_amd import cdc
    from tests.cdc_f64 import loss_f64, random_feats
    tgt, src = random_feats(FEAT_SHAPES, 4, seed=sum(layers))
    tgt[1] = tgt[1].contiguous(memory_format=torch.channels_last)      # the generator's layout
    src[1] = src[1].contiguous(memory_format=torch.channels_last)
    used = sorted(set(layers))
    t64 = [f.double().requires_grad_(True) for f in tgt]
    ref = loss_f64(t64, src, layers)
    gref = torch.autograd.grad(ref, [t64[l] for l in used])
    t32 = [f.clone().requires_grad_(True) for f in tgt]
    cpu = _loss_fp32(t32, src, layers)
    gcpu = torch.autograd.grad(cpu, [t32[l] for l in used])
    td = [f.to(DEV).requires_grad_(True) for f in tgt]
    loss = cdc.distance_consistency_loss(td, [f.to(DEV) for f in src], layers)
    gdev = torch.autograd.grad(loss, [td[l] for l in used])
    assert loss.dtype == torch.float32 and loss.dim() == 0
    err, base = abs(float(loss.detach()) - float(ref.detach())), abs(float(cpu.detach()) - float(ref.detach()))
    print(f'loss {layers}: value {float(ref.detach()):.6e}  device err {err:.3e}  fp32 composition {base:.3e}')
    assert err <= 4 * base
    for l, a, b, r in zip(used, gdev, gcpu, gref):
        scale = r.abs().max()
        e, bs = float((a.double().cpu() - r).abs().max() / scale), float((b.double() - r).abs().max() / scale)
        print(f'  d loss / d feats[{l}]: device {e:.3e}  fp32 composition {bs:.3e}  bound {4 * bs:.3e}')
        assert a.stride() == td[l].stride()
        assert e <= 4 * bs


def test_batch_of_two_is_exactly_zero():
    from rick_amd import cdc
    from tests.cdc_f64 import random_feats
    tgt, src = random_feats(FEAT_SHAPES, 2, seed=5)
    td = [f.to(DEV).requires_grad_(True) for f in tgt]
    loss = cdc.distance_consistency_loss(td, [f.to(DEV) for f in src], [1, 3])
    assert float(loss.detach()) == 0.0
    for g in torch.autograd.grad(loss, [td[1], td[3]]):
        assert not g.any()


# ---- generator and trainer -------------------------------------------------------------------------------------------------------
def _build(size=32):
    from rick_amd.models import Discriminator, Generator
    torch.manual_seed(11)
    g0, d0 = Generator(size, 512, 2), Discriminator(size)

    def make(perturb=0.0):
        g, d = Generator(size, 512, 2), Discriminator(size)
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


def _noise_maps(g):
    gen = torch.Generator(DEV).manual_seed(2)
    return [torch.randn(n.shape, device=DEV, generator=gen) for n in g.make_noise()]


def _loss_composed(feats_t, feats_s, layers, dtype):
    """The loss by torch composition on the device, on the SAME feature tensors, in `dtype` throughout."""
    def cosines(feats):
        rows = []
        for i, l in enumerate(layers):
            X = feats[l].flatten(1).to(dtype)
            G = X @ X.t()
            n = torch.diagonal(G).sqrt().clamp_min(1e-8)
            c = G[i] / (n[i] * n)
            rows.append(torch.cat([c[:i], c[i + 1:]]))
        return torch.stack(rows)
    with torch.no_grad():
        lps = torch.log_softmax(cosines(feats_s), 1)
    return (lps.exp() * (lps - torch.log_softmax(cosines(feats_t), 1))).mean()


def test_generator_parameter_gradients_end_to_end():
    """32 px, batch 4, fixed noise maps: d loss / d (every trained generator parameter) with the loss on the Gram kernels against
    the same loss rebuilt in fp64 by torch composition on the same feature tensors (one forward pass, so the convolutions and
    their backward kernels are common to both), bounded by four times the error of the fp32 composition."""
    from rick_amd import cdc
    from rick_amd.train import g_optim_filter
    make = _build()
    g, _ = make(perturb=0.3)
    src, _ = make()
    params = []
    for n, p in g.named_parameters():
        p.requires_grad = g_optim_filter(n)
        if p.requires_grad:
            params.append((n, p))
    z = torch.randn(4, 512, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    noise, layers = _noise_maps(g), [1, 3, 3, 5]
    with torch.no_grad():
        _, fs = src([z], noise=noise, return_feats=True)
    _, ft = g([z], noise=noise, return_feats=True)
    assert len(ft) == g.n_latent - 1
    ps = [p for _, p in params]
    gd = torch.autograd.grad(cdc.distance_consistency_loss(ft, fs, layers), ps, retain_graph=True, allow_unused=True)
    g64 = torch.autograd.grad(_loss_composed(ft, fs, layers, torch.float64), ps, retain_graph=True, allow_unused=True)
    g32 = torch.autograd.grad(_loss_composed(ft, fs, layers, torch.float32), ps, allow_unused=True)
    seen, worst = 0, (0.0, 0.0)
    for (n, _), a, r, b in zip(params, gd, g64, g32):
        assert (a is None) == (r is None), n
        if r is None or not r.any():
            continue
        seen += 1
        scale = r.double().abs().max()
        e, bs = float((a.double() - r.double()).abs().max() / scale), float((b.double() - r.double()).abs().max() / scale)
        worst = max(worst, (e, bs))
        assert e <= 4 * bs, (n, e, bs)
    print(f'generator parameters ({seen} tensors): worst device err {worst[0]:.3e} with fp32 composition {worst[1]:.3e}')
    assert seen >= 8


def _trainer(make, weight, source=True, graphs=False):
    from rick_amd.train import RickTrainer, TrainConfig
    g, d = make(perturb=0.3)
    g_ema, d_ema = make()
    src = make()[0] if source else None
    tr = RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, cdc_weight=weight, cdc_batch=4), g, d, g_ema, d_ema,
                     g_source=src)
    if graphs:
        tr.enable_graphs(True)
    return tr, src


def _fixed(g):
    gen = torch.Generator(DEV).manual_seed(7)
    return dict(noise=[torch.randn(2, 512, device=DEV, generator=gen)], g_noise=_noise_maps(g),
                cdc_noise=torch.randn(4, 512, device=DEV, generator=gen), cdc_layers=[2, 4, 2, 1])


def _params(net):
    return {n: p.detach().clone() for n, p in net.named_parameters()}


def test_g_step_with_the_term_eager_and_graph_flag_agree():
    """The loss value of the step equals the stand-alone loss on the same inputs; g_source is untouched; graph=True takes the eager
    path while the term is on (nothing is captured) and leaves the same parameters bit for bit, step after step."""
    from rick_amd import cdc
    make = _build()
    a, src = _trainer(make, 1000.0)
    b, _ = _trainer(make, 1000.0, graphs=True)
    fx = _fixed(a.g)
    with torch.no_grad():
        alone = cdc.distance_consistency_loss(a.g([fx['cdc_noise']], noise=fx['g_noise'], return_feats=True)[1],
                                              src([fx['cdc_noise']], noise=fx['g_noise'], return_feats=True)[1], fx['cdc_layers'])
    before = copy.deepcopy(src.state_dict())
    start = _params(a.g)
    for k in range(4):                                         # a captured step would replay from the third call on
        a.g_step(fx['noise'], fx['g_noise'], cdc_noise=fx['cdc_noise'], cdc_layers=fx['cdc_layers'])
        b.g_step(fx['noise'], fx['g_noise'], graph=True, cdc_noise=fx['cdc_noise'], cdc_layers=fx['cdc_layers'])
        if k == 0:
            assert float(alone) > 0 and torch.equal(a.losses['cdc'], alone)
        assert torch.equal(a.losses['cdc'], b.losses['cdc']) and torch.equal(a.losses['g'], b.losses['g'])
        pa, pb = _params(a.g), _params(b.g)
        assert all(torch.equal(pa[n], pb[n]) for n in pa)
    assert 'graphs' not in b._gs.get('g', {})
    assert any(not torch.equal(start[n], pa[n]) for n in pa)
    assert all(torch.equal(before[k], v) for k, v in src.state_dict().items())
    assert all(p.grad is None and not p.requires_grad for p in src.parameters()) and not src.training
    b.g_step(None, None, graph=True)                           # the training loop's call: no noise given, drawn by the step
    assert torch.isfinite(b.losses['cdc']) and torch.isfinite(b.losses['g'])


def test_g_step_gradient_is_the_sum_of_both_terms():
    """Wiring: the flat gradient of a step with the term equals the plain step's plus weight times the term's own gradient.  The
    two sides add the same fp32 contributions in another order and scale by the weight at another place; 1e-3 of a tensor's
    largest gradient entry (the agreement smoke() asks of a whole step against its oracle) separates that from a missing or
    doubled term, which is an error of order one."""
    from rick_amd.train import g_optim_filter
    make = _build()
    w = 64.0
    on, _ = _trainer(make, w)
    off, _ = _trainer(make, 0.0)
    ref, _ = _trainer(make, w)
    fx = _fixed(on.g)
    on.g_step(fx['noise'], fx['g_noise'], cdc_noise=fx['cdc_noise'], cdc_layers=fx['cdc_layers'])
    off.g_step(fx['noise'], fx['g_noise'])
    named = [(n, p) for n, p in ref.g.named_parameters() if g_optim_filter(n)]
    (cdc_term,) = ref.g_terms                                  # the only term that is on (rick_amd/gterms.py)
    _, value = cdc_term({k: fx[k] for k in cdc_term.draws}, fx['g_noise'], {})['cdc']
    term = torch.autograd.grad(value, [p for _, p in named], allow_unused=True)
    g_on = {n: p.grad for n, p in on.g.named_parameters()}
    g_off = {n: p.grad for n, p in off.g.named_parameters()}
    moved = 0
    for (n, _), t in zip(named, term):
        want = g_off[n] if t is None else g_off[n] + w * t
        assert float((g_on[n] - want).abs().max()) <= 1e-3 * float(want.abs().max()), n
        moved += t is not None and bool((w * t).abs().max() > 1e-2 * g_off[n].abs().max())
    assert moved >= 4                                          # the term is a visible part of the gradient it is checked in


def test_zero_weight_changes_nothing():
    make = _build()
    with_src, src = _trainer(make, 0.0)
    without, _ = _trainer(make, 0.0, source=False)
    fx = _fixed(with_src.g)
    for tr in (with_src, without):
        tr.g_step(fx['noise'], fx['g_noise'])
    assert 'cdc' not in with_src.losses
    pa, pb = _params(with_src.g), _params(without.g)
    assert all(torch.equal(pa[n], pb[n]) for n in pa)
    assert torch.equal(with_src.losses['g'], without.losses['g'])
