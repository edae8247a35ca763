"""The trainer with CDC's patch-level discriminator and anchor sampling (rick_amd/patchd.py, TrainConfig.subspace_freq): off means
untouched, a patch D step moves the trunk up to the exit and the tap's head and nothing else, a patch G step moves the generator
alone, `graph=True` runs such steps eagerly with the same result, and anchor iterations draw their latents around the anchors.
32 px, batch 2, built as tests/test_gpu_cdc.py builds its networks."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _build(size=32):
    from rick_amd.models import Discriminator, Generator
    from rick_amd.patchd import PatchHeads
    torch.manual_seed(11)
    g0, d0, h0 = Generator(size, 512, 2), Discriminator(size), PatchHeads(n_heads=3)

    def make():
        g, d = Generator(size, 512, 2), Discriminator(size)
        g.load_state_dict(g0.state_dict())
        d.load_state_dict(d0.state_dict())
        return g.to(DEV), d.to(DEV)
    return make, h0


def _trainer(make, heads=None, graphs=False, **cfg):
    from rick_amd.train import RickTrainer, TrainConfig
    g, d = make()
    g_ema, d_ema = make()
    tr = RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, **cfg), g, d, g_ema, d_ema,
                     patch_heads=None if heads is None else copy.deepcopy(heads).to(DEV))
    if graphs:
        tr.enable_graphs(True)
    return tr


def _fixed(g):
    gen = torch.Generator(DEV).manual_seed(7)
    maps = [torch.randn(n.shape, device=DEV, generator=gen) for n in g.make_noise()]
    return dict(noise=[torch.randn(2, 512, device=DEV, generator=gen)], g_noise=maps,
                real=torch.randn(2, 3, 32, 32, device=DEV, generator=gen).clamp_(-1, 1))


def _params(net):
    return {n: p.detach().clone() for n, p in net.named_parameters()}


def _changed(before, net):
    return {n for n, p in net.named_parameters() if not torch.equal(before[n], p.detach())}


def test_feature_off_changes_nothing():
    make, _ = _build()
    plain = _trainer(make)
    off = _trainer(make, subspace_freq=0, subspace_std=0.3, feat_ind=2, n_anchors=5)
    fx = _fixed(plain.g)
    for tr in (plain, off):
        tr.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'])
        tr.g_step(fx['noise'], fx['g_noise'])
    assert off.patch_heads is None and off.anchors is None and off.last_patch is None
    for a, b in ((plain.d, off.d), (plain.g, off.g)):
        pa, pb = _params(a), _params(b)
        assert all(torch.equal(pa[n], pb[n]) for n in pa)
    assert torch.equal(plain.losses['d'], off.losses['d']) and torch.equal(plain.losses['g'], off.losses['g'])


def test_patch_d_step_moves_the_trunk_up_to_the_exit_and_one_head():
    """p_ind 0 at 32 px is b1.t1: the path is convs.0 (owned by no optimiser) and convs.1.conv1."""
    make, heads = _build()
    tr = _trainer(make, heads, subspace_freq=4)
    fx = _fixed(tr.g)
    d0, h0, g0 = _params(tr.d), _params(tr.patch_heads), _params(tr.g)
    loss = tr.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'], patch=0)
    assert torch.isfinite(loss) and float(loss) > 0
    moved = _changed(d0, tr.d)
    assert moved == {'convs.1.conv1.0.weight', 'convs.1.conv1.1.bias'}        # everything behind the exit block: bit-unchanged
    assert _changed(h0, tr.patch_heads) == {'new_conv.0.0.weight', 'new_conv.0.1.bias'}
    assert not _changed(g0, tr.g)
    assert tr.head_optim.steps == [1] * 6 and tr.ada.n == 0
    # a t2 tap takes the whole exit block
    d1, h1 = _params(tr.d), _params(tr.patch_heads)
    tr.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'], patch=1)
    moved = _changed(d1, tr.d)
    assert {'convs.1.conv1.0.weight', 'convs.1.conv2.1.weight', 'convs.1.conv2.2.bias'} <= moved
    assert all(n.startswith('convs.1.') for n in moved)
    assert _changed(h1, tr.patch_heads) == {'new_conv.1.0.weight', 'new_conv.1.1.bias'}


def test_patch_g_step_moves_the_generator_alone():
    make, heads = _build()
    tr = _trainer(make, heads, subspace_freq=4)
    fx = _fixed(tr.g)
    d0, h0, g0 = _params(tr.d), _params(tr.patch_heads), _params(tr.g)
    loss = tr.g_step(fx['noise'], fx['g_noise'], patch=2)
    assert torch.isfinite(loss) and float(loss) > 0
    assert len(_changed(g0, tr.g)) >= 8
    assert not _changed(d0, tr.d) and not _changed(h0, tr.patch_heads)
    assert all(p.requires_grad for p in tr.patch_heads.parameters())           # the freeze of the step is undone


def test_graph_flag_and_eager_patch_steps_agree():
    """graph=True with the feature on runs D and G steps eagerly (nothing is captured) and leaves the same parameters bit for bit,
    call after call (a captured step would replay from the third call on)."""
    make, heads = _build()
    a = _trainer(make, heads, subspace_freq=4)
    b = _trainer(make, heads, graphs=True, subspace_freq=4)
    fx = _fixed(a.g)
    for k in range(4):
        p = k % 3
        a.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'], patch=p)
        b.d_step(fx['real'], fx['noise'], g_noise=fx['g_noise'], graph=True, patch=p)
        a.g_step(fx['noise'], fx['g_noise'], patch=p)
        b.g_step(fx['noise'], fx['g_noise'], graph=True, patch=p)
        assert torch.equal(a.losses['d'], b.losses['d']) and torch.equal(a.losses['g'], b.losses['g'])
        for na, nb in ((a.d, b.d), (a.g, b.g), (a.patch_heads, b.patch_heads)):
            pa, pb = _params(na), _params(nb)
            assert all(torch.equal(pa[n], pb[n]) for n in pa)
    assert 'graphs' not in b._gs.get('d', {}) and 'graphs' not in b._gs.get('g', {})
    b.d_step(fx['real'], None, graph=True)                                     # image-level, no noise given: drawn by the step, eager
    assert 'graphs' not in b._gs.get('d', {}) and torch.isfinite(b.losses['d'])


@pytest.mark.parametrize('std', [0.05, 0.0])
def test_anchor_iteration_draws_latents_around_the_anchors(std):
    make, heads = _build()
    tr = _trainer(make, heads, subspace_freq=4, subspace_std=std, n_anchors=5)
    assert tr.anchors.shape == (5, 512) and tr.anchors.device.type == 'cuda'
    seen, inner = [], tr.g.forward

    def recording(styles, **kw):
        if not kw.get('input_is_latent'):
            seen.append(styles)
        return inner(styles, **kw)
    tr.g.forward = recording
    real = _fixed(tr.g)['real']
    tr.iteration(0, real)
    assert tr.last_patch == (0, None) and len(seen) == 2                       # the D step's fakes and the G step's
    for styles in seen:
        assert len(styles) == 1 and styles[0].shape == (2, 512)
        dist = torch.cdist(styles[0], tr.anchors).min(1).values
        if std == 0:
            assert all(any(torch.equal(r, a) for a in tr.anchors) for r in styles[0])
        else:
            assert bool((dist <= 6 * std * 512 ** 0.5).all()) and bool((dist > 0).all())
    del seen[:]
    tr.iteration(1, real)                                                      # a patch iteration: random latents, one tap in both steps
    which, p_ind = tr.last_patch
    assert which == 1 and 0 <= p_ind < 3 and len(seen) == 2
    assert all(torch.isfinite(tr.losses[k]) for k in ('d', 'g'))
