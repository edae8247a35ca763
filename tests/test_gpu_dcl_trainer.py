"""The trainer's G step and D step with DCL's contrastive terms (rick_amd/dcl.py) at 32 px, n_mlp = 2, batch 4.

Parameter gradients follow the fourfold rule of tests/test_gpu_cdc.py: the term on the cross-Gram kernels against the same
term rebuilt in fp64 by torch composition on the SAME feature tensors (one forward pass, so the convolutions and their backward
kernels are common to both), bounded by four times the error of the fp32 composition."""
import copy

import pytest
import torch

from tests.test_gpu_dcl import cl1_composed, cl2_composed

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = 4


def _build(size=32):
    from rick_amd.models import Discriminator, Generator
    torch.manual_seed(11)
    g0, d0 = Generator(size, 512, 2), Discriminator(size)

    def make(perturb=0.0):
        g, d = Generator(size, 512, 2), Discriminator(size)
        g.load_state_dict(g0.state_dict())
        d.load_state_dict(d0.state_dict())
        if perturb:                                            # the adapted networks have moved away from the source
            gen = torch.Generator().manual_seed(1)
            with torch.no_grad():
                for net in (g, d):
                    for n, p in net.named_parameters():
                        if n.startswith('convs.'):
                            p.add_(perturb * p.abs().mean() * torch.randn(p.shape, generator=gen))
        return g.to(DEV), d.to(DEV)
    return make


def _trainer(make, g_weight=0.0, d_weight=0.0, sources=True, graphs=False):
    from rick_amd.train import RickTrainer, TrainConfig
    g, d = make(perturb=0.3)
    g_ema, d_ema = make()
    gs, ds = make() if sources else (None, None)
    cfg = TrainConfig(size=32, batch=B, n_mlp=2, warmup_iter=0, dcl_g_weight=g_weight, dcl_d_weight=d_weight, dcl_batch=B)
    tr = RickTrainer(cfg, g, d, g_ema, d_ema, g_source=gs, d_source=ds)
    if graphs:
        tr.enable_graphs(True)
    return tr, gs, ds


def _fixed(g):
    gen = torch.Generator(DEV).manual_seed(7)
    return dict(noise=[torch.randn(B, 512, device=DEV, generator=gen), torch.randn(B, 512, device=DEV, generator=gen)],
                g_noise=[torch.randn(B, *n.shape[1:], device=DEV, generator=gen) for n in g.make_noise()],
                real=torch.rand(B, 3, 32, 32, device=DEV, generator=gen) * 2 - 1,
                z=torch.randn(B, 512, device=DEV, generator=gen))


def _params(net):
    return {n: p.detach().clone() for n, p in net.named_parameters()}


def _fourfold(named, gd, g64, g32, least):
    seen, worst = 0, (0.0, 0.0)
    for (n, _), a, r, b in zip(named, gd, g64, g32):
        assert (a is None) == (r is None), n
        if r is None or not r.any():
            continue
        seen += 1
        scale = r.double().abs().max()
        e, bs = float((a.double() - r.double()).abs().max() / scale), float((b.double() - r.double()).abs().max() / scale)
        worst = max(worst, (e, bs))
        assert e <= 4 * bs, (n, e, bs)
    assert seen >= least, seen
    return seen, worst


def test_g_step_term_parameter_gradients_and_value():
    from rick_amd import dcl
    from rick_amd.train import g_optim_filter
    make = _build()
    tr, gs, _ = _trainer(make, g_weight=2.0)
    fx = _fixed(tr.g)
    layers = [1, 3, 3, 5]
    named = [(n, p) for n, p in tr.g.named_parameters() if g_optim_filter(n)]
    ps = [p for _, p in named]
    ft, fs = tr._feature_pair(fx['z'], fx['g_noise'])
    assert len(ft) == tr.g.n_latent - 1 and not any(f.requires_grad for f in fs)
    (dcl_term,) = tr.g_terms                                   # the only term that is on (rick_amd/gterms.py)
    _, term = dcl_term({'dcl_layers': layers}, None, {dcl_term: (ft, fs)})['dcl_g']     # on this pair, as if it were handed on
    gd = torch.autograd.grad(term, ps, retain_graph=True, allow_unused=True)
    g64 = torch.autograd.grad(cl1_composed(ft, fs, layers, torch.float64), ps, retain_graph=True, allow_unused=True)
    g32 = torch.autograd.grad(cl1_composed(ft, fs, layers, torch.float32), ps, allow_unused=True)
    seen, worst = _fourfold(named, gd, g64, g32, 8)
    print(f'CL1, generator parameters ({seen} tensors): worst device err {worst[0]:.3e} with fp32 composition {worst[1]:.3e}')
    # the step: the recorded loss is the stand-alone loss on the same draws, the source generator is untouched
    before = copy.deepcopy(gs.state_dict())
    start = _params(tr.g)
    tr.g_step(fx['noise'][:1], fx['g_noise'], dcl_noise=fx['z'], dcl_layers=layers)
    assert float(term.detach()) > 0 and torch.equal(tr.losses['dcl_g'], term.detach()) and 'cdc' not in tr.losses
    after = _params(tr.g)
    assert any(not torch.equal(start[n], after[n]) for n in after)
    assert all(torch.equal(before[k], v) for k, v in gs.state_dict().items())
    assert all(p.grad is None and not p.requires_grad for p in gs.parameters())
    assert dcl.TAU == tr.cfg.dcl_tau


def _d_forward(tr, gs, ds, fx, inject):
    """What the D step computes before its loss, on the trainer's networks: the feature lists of anchors, positives, negatives."""
    with torch.no_grad():
        fake, _ = tr.g(fx['noise'], noise=fx['g_noise'], inject_index=inject)
        pos = ds(gs(fx['noise'], noise=fx['g_noise'], inject_index=inject)[0])[1]
        x = torch.cat([fake, fx['real']], 0)
    pred, feats = tr.d(x, calls=2)
    return pred, [f[:B] for f in feats], pos, [f[B:] for f in feats]


def test_d_step_term_parameter_gradients():
    from rick_amd import dcl
    from rick_amd.train import d_optim_filter
    make = _build()
    tr, gs, ds = _trainer(make, d_weight=0.5)
    fx = _fixed(tr.g)
    tr._set_d_stage(10 ** 9)
    named = [(n, p) for n, p in tr.d.named_parameters() if d_optim_filter(n)]
    ps = [p for _, p in named]
    _, anc, pos, neg = _d_forward(tr, gs, ds, fx, 3)
    assert len(anc) == 8 and not any(f.requires_grad for f in pos)            # 1 + 2 * 3 + 1 features at 32 px
    layers = [0, 4, 7, 4]                                                        # the input conv, a block's t2 (twice), the final conv
    gd = torch.autograd.grad(dcl.discriminator_contrastive_loss(anc, pos, neg, layers, tr.cfg.dcl_tau), ps, retain_graph=True,
                             allow_unused=True)
    g64 = torch.autograd.grad(cl2_composed(anc, pos, neg, layers, torch.float64), ps, retain_graph=True, allow_unused=True)
    g32 = torch.autograd.grad(cl2_composed(anc, pos, neg, layers, torch.float32), ps, allow_unused=True)
    seen, worst = _fourfold(named, gd, g64, g32, 8)
    print(f'CL2, discriminator parameters ({seen} tensors): worst device err {worst[0]:.3e} with fp32 composition {worst[1]:.3e}')


def test_d_step_reaches_the_discriminator_only_and_shares_the_draws():
    from rick_amd import dcl
    make = _build()
    tr, gs, ds = _trainer(make, d_weight=0.5)
    fx = _fixed(tr.g)
    layers = [1, 3, 3, 6]                                                        # t1 and t2 of fused blocks among them
    tr._set_d_stage(10 ** 9)
    _, anc, pos, neg = _d_forward(tr, gs, ds, fx, 3)
    alone = dcl.discriminator_contrastive_loss(anc, pos, neg, layers, tr.cfg.dcl_tau).detach()
    seen = {}
    for name, net in (('t', tr.g), ('s', gs)):
        def recording(styles, _inner=net.forward, _name=name, **kw):
            seen[_name] = (styles, kw.get('inject_index'), kw.get('noise'))
            return _inner(styles, **kw)
        net.forward = recording
    frozen = {k: _params(n) for k, n in (('g', tr.g), ('gs', gs), ('ds', ds))}
    g_grad = tr.g_flat.grad.clone()
    d_start = _params(tr.d)
    tr.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'], dcl_layers=layers, dcl_inject=3)
    assert float(alone) > 0 and torch.equal(tr.losses['dcl_d'], alone)
    # G_t and G_s: the same latents, the same mixing index, the same noise maps
    assert seen['t'][1] == seen['s'][1] == 3 and seen['t'][0] is seen['s'][0]
    assert len(seen['t'][2]) == len(fx['g_noise']) and all(a is b for a, b in zip(seen['t'][2], seen['s'][2]))
    for k, net in (('g', tr.g), ('gs', gs), ('ds', ds)):                         # no generator and no source network moves
        assert all(torch.equal(frozen[k][n], p) for n, p in net.named_parameters()), k
    assert torch.equal(g_grad, tr.g_flat.grad)
    assert all(p.grad is None and not p.requires_grad for net in (gs, ds) for p in net.parameters())
    d_after = _params(tr.d)
    assert any(not torch.equal(d_start[n], d_after[n]) for n in d_after)
    # the draws when none are given: one index and one set of maps, handed to both
    seen.clear()
    tr.d_step(fx['real'], fx['noise'])
    assert seen['t'][1] is not None and seen['t'][1] == seen['s'][1] and 1 <= seen['t'][1] < tr.g.n_latent
    assert all(a is b for a, b in zip(seen['t'][2], seen['s'][2])) and len(seen['t'][2]) == tr.g.num_layers
    assert torch.isfinite(tr.losses['dcl_d'])


def test_d_step_gradient_is_the_sum_of_both_terms():
    """Wiring, as tests/test_gpu_cdc.py checks it for the G step: the flat gradient of a step with the term equals the plain
    step's plus weight times the term's own gradient.  The two sides add the same fp32 contributions in another order; 1e-3 of a
    tensor's largest gradient entry separates that from a missing or doubled term, which is an error of order one."""
    from rick_amd import dcl
    from rick_amd.train import d_optim_filter
    make = _build()
    w, layers = 0.5, [1, 3, 3, 6]
    on, _, _ = _trainer(make, d_weight=w)
    off, _, _ = _trainer(make)
    ref, gs, ds = _trainer(make, d_weight=w)
    fx = _fixed(on.g)
    on.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'], dcl_layers=layers, dcl_inject=3)
    off.g.forward = (lambda styles, _inner=off.g.forward, **kw: _inner(styles, inject_index=3, **kw))
    off.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'])
    ref._set_d_stage(10 ** 9)
    named = [(n, p) for n, p in ref.d.named_parameters() if d_optim_filter(n)]
    _, anc, pos, neg = _d_forward(ref, gs, ds, fx, 3)
    term = torch.autograd.grad(dcl.discriminator_contrastive_loss(anc, pos, neg, layers, ref.cfg.dcl_tau), [p for _, p in named],
                               allow_unused=True)
    g_on = {n: p.grad for n, p in on.d.named_parameters()}
    g_off = {n: p.grad for n, p in off.d.named_parameters()}
    moved = 0
    for (n, _), t in zip(named, term):
        want = g_off[n] if t is None else g_off[n] + w * t
        assert float((g_on[n] - want).abs().max()) <= 1e-3 * float(want.abs().max()), n
        moved += t is not None and bool((w * t).abs().max() > 1e-2 * g_off[n].abs().max())
    assert moved >= 4                                                            # the term is a visible part of the gradient


def test_steps_with_a_term_run_eagerly_under_graph_true():
    make = _build()
    a, _, _ = _trainer(make, g_weight=2.0, d_weight=0.5)
    b, _, _ = _trainer(make, g_weight=2.0, d_weight=0.5, graphs=True)
    fx = _fixed(a.g)
    kd = dict(g_noise=fx['g_noise'], dcl_layers=[1, 3, 3, 6], dcl_inject=3)
    kg = dict(dcl_noise=fx['z'], dcl_layers=[2, 4, 2, 1])
    for k in range(4):                                                           # a captured step would replay from the third call on
        a.d_step(fx['real'], fx['noise'], **kd)
        b.d_step(fx['real'], fx['noise'], graph=True, **kd)
        a.g_step(fx['noise'][:1], fx['g_noise'], **kg)
        b.g_step(fx['noise'][:1], fx['g_noise'], graph=True, **kg)
        for key in ('d', 'dcl_d', 'g', 'dcl_g'):
            assert torch.equal(a.losses[key], b.losses[key]), (k, key)
        for na, nb in ((a.g, b.g), (a.d, b.d)):
            pa, pb = _params(na), _params(nb)
            assert all(torch.equal(pa[n], pb[n]) for n in pa)
    assert 'graphs' not in b._gs.get('d', {}) and 'graphs' not in b._gs.get('g', {})
    b.d_step(fx['real'], None, graph=True)                                       # the training loop's calls: noise drawn by the step
    b.g_step(None, graph=True)
    assert torch.isfinite(b.losses['dcl_d']) and torch.isfinite(b.losses['dcl_g'])


def test_zero_weights_change_nothing():
    make = _build()
    with_src, _, _ = _trainer(make)
    without, _, _ = _trainer(make, sources=False)
    fx = _fixed(with_src.g)
    for tr in (with_src, without):
        tr.g.forward = (lambda styles, _inner=tr.g.forward, **kw: _inner(styles, **{'inject_index': 3, **kw}))
        tr.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'])
        tr.g_step(fx['noise'], fx['g_noise'])
    assert 'dcl_g' not in with_src.losses and 'dcl_d' not in with_src.losses
    for na, nb in ((with_src.g, without.g), (with_src.d, without.d)):
        pa, pb = _params(na), _params(nb)
        assert all(torch.equal(pa[n], pb[n]) for n in pa)
    assert torch.equal(with_src.losses['g'], without.losses['g']) and torch.equal(with_src.losses['d'], without.losses['d'])


def test_g_step_with_every_term_on_is_the_sum_of_the_terms():
    """All extra terms of the G step together (rick_amd/gterms.py): distance consistency and CL1 on one shared forward pair, then
    both CLIP-space terms on the tiny image configuration A.  Every draw and noise map is pinned.  Wiring, by the rule and the
    bound of tests/test_gpu_cdc.py::test_g_step_gradient_is_the_sum_of_both_terms: each optimiser-owned tensor of the flat
    gradient equals the plain step's plus the sum of weight times each term's own gradient, within 1e-3 of the tensor's largest
    wanted entry (the two sides add the same fp32 contributions in another order; a missing or doubled term is an error of
    order one).  The weights make every term at least 1e-2 of the adversarial gradient on four tensors or more: measured, on all
    20 tensors of convs.0 ... convs.3 the smallest of the four ratios lies between 3.1e-2 and 2.8e-1 (the distance-consistency
    term 3.7e-2 ... 1.2, CL1 0.12 ... 4.4, clip_dir 3.1e-2 ... 8.2, clip_within 0.17 ... 4.0; no feature list reaches convs.5
    and the drawn layers leave convs.4 out of the distance-consistency term), and the largest error of the 30 is 5.9e-6."""
    from rick_amd.clipguide import ClipGuide
    from rick_amd.train import RickTrainer, TrainConfig, g_optim_filter
    from tests.test_gpu_clip import network
    from tests.test_gpu_clip_grad import _guide_inputs
    make = _build()
    weights = dict(cdc_weight=2048.0, dcl_g_weight=64.0, clip_dir_weight=0.25, clip_within_weight=0.25)

    def trainer(**w):
        g, d = make(perturb=0.3)
        g_ema, d_ema = make()
        cfg = TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, cdc_batch=4, dcl_batch=4, clip_batch=2, **w)
        return RickTrainer(cfg, g, d, g_ema, d_ema, g_source=make()[0], clip=ClipGuide(network('A'), _guide_inputs()[2]))
    on, off, ref = trainer(**weights), trainer(), trainer(**weights)
    assert [type(t).__name__ for t in on.g_terms] == ['CdcTerm', 'DclGTerm', 'ClipTerm'] and off.g_terms == []
    gen = torch.Generator(DEV).manual_seed(7)
    noise = [torch.randn(2, 512, device=DEV, generator=gen)]
    g_noise = [torch.randn(n.shape, device=DEV, generator=gen) for n in on.g.make_noise()]
    draws = dict(cdc_noise=torch.randn(4, 512, device=DEV, generator=gen), cdc_layers=[2, 4, 2, 1], dcl_layers=[1, 3, 3, 5],
                 clip_noise=torch.randn(2, 512, device=DEV, generator=gen))
    source_calls = []
    on.g_source.register_forward_hook(lambda mod, args, out: source_calls.append(args[0][0].shape[0]))
    on.g_step(noise, g_noise, **draws)
    off.g_step(noise, g_noise)
    assert source_calls == [4, 2]                                                # the shared pair, then the CLIP terms' images
    names = ('cdc', 'dcl_g', 'clip_dir', 'clip_within')
    assert all(n in on.losses and torch.isfinite(on.losses[n]) for n in names) and not any(n in off.losses for n in names)
    named = [(n, p) for n, p in ref.g.named_parameters() if g_optim_filter(n)]
    own = {}
    for name in names:                      # one evaluation per loss: the CLIP encoder keeps the activations of one backward pass
        memo, found = {}, {}
        for term in ref.g_terms:
            found.update(term(draws, g_noise, memo))
        weight, value = found[name]
        assert weight == weights[name + '_weight'] and torch.equal(value.detach(), on.losses[name])
        own[name] = [None if t is None else weight * t
                     for t in torch.autograd.grad(value, [p for _, p in named], allow_unused=True)]
    g_on = {n: p.grad for n, p in on.g.named_parameters()}
    g_off = {n: p.grad for n, p in off.g.named_parameters()}
    moved = 0
    for k, (n, _) in enumerate(named):
        want = g_off[n].clone()
        ratios = []
        for name in names:
            t = own[name][k]
            if t is not None:
                want += t
            ratios.append(0.0 if t is None else float(t.abs().max() / g_off[n].abs().max()))
        err = float((g_on[n] - want).abs().max()) / float(want.abs().max())
        print(f'{n}: err {err:.3e}; term / adversarial gradient ' + ', '.join(f'{a} {r:.3e}' for a, r in zip(names, ratios)))
        assert err <= 1e-3, n
        moved += min(ratios) > 1e-2
    assert moved >= 4                                                            # every term is a visible part of the gradient
