"""The trainer with DiffAugment (TrainConfig.diffaug): an eager D / R1 / G sequence against the same sequence on the fp64 host
closed form, graph replay against eager with changing draws, and the field left empty."""
import pytest
import torch

from tests import diffaug_f64 as O

pytestmark = pytest.mark.gpu

POLICY = 'color,translation,cutout'


class _Source:
    """Pinned draws for RickTrainer.diffaug_source: call k draws its records from seed 1000 + k."""

    def __init__(self, tr):
        self.tr, self.k, self.log = tr, 0, []

    def __call__(self, n):
        from rick_amd.diffaug import draw_params
        size = self.tr.cfg.size
        rec = draw_params(n, size, size, POLICY, generator=torch.Generator().manual_seed(1000 + self.k))
        self.k += 1
        self.log.append(rec)
        return rec


def _trainer(size, B, **kw):
    from rick_amd.train import RickTrainer, TrainConfig
    from tests.test_gpu_models import build
    g, d = build(size)
    tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, diffaug=POLICY, **kw), g, d, *build(size))
    tr.diffaug_source = _Source(tr)
    return tr


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_eager_diffaug_steps_match_the_fp64_closed_form(monkeypatch):
    """D on DiffAugment(cat(fake, real)), R1 on D(DiffAugment(real)) w.r.t. the plain reals (the whole closed family under
    second_order), G through the op — against the same trainer with the fused op replaced by the fp64 host closed form as a
    differentiable torch composition, for the same draws: losses and flat gradients of every step to 1e-5."""
    import rick_amd.train as T
    from rick_amd.synth import synth_latents, synth_reals, synth_tensor
    size, B = 32, 2
    z, real = synth_latents(B, seed=41).cuda(), synth_reals(B, size=size, seed=42).cuda()

    def composed_for(src):
        def comp(t, rec):
            return O.apply(t.double().cpu(), rec).float().to(t.device)

        def op(x, params):
            if x.shape[0] == 2 * B:                   # D step: cat(fake, real), drawn real first
                real_rec, fake_rec = src.log[-2:]
                return torch.cat([comp(x[:B], fake_rec), comp(x[B:], real_rec)])
            return comp(x, src.log[-1])
        return op

    def run(with_composed):
        tr = _trainer(size, B)
        if with_composed:
            monkeypatch.setattr(T, 'diffaug_fused', composed_for(tr.diffaug_source))
        noises = [synth_tensor(f'daugnoise/{i}', tuple(getattr(tr.g.noises, f'noise_{i}').shape)).cuda() for i in range(tr.g.num_layers)]
        out = []
        for step in (lambda: tr.d_step(real, [z], g_noise=noises), lambda: tr.r1_step(real), lambda: tr.g_step([z], g_noise=noises)):
            loss = step().clone()
            out.append((loss, tr.d_flat.grad.clone(), tr.g_flat.grad.clone()))
        monkeypatch.undo()
        return tr, out
    fused, a = run(False)
    comp_tr, b = run(True)
    assert len(fused.diffaug_source.log) == 4
    assert all(x.tobytes() == y.tobytes() for x, y in zip(fused.diffaug_source.log, comp_tr.diffaug_source.log))
    for name, (la, da, ga), (lb, db, gb) in zip(('d', 'r1', 'g'), a, b):
        grad_a, grad_b = (ga, gb) if name == 'g' else (da, db)
        print(f'diffaug trainer {name}: loss rel {_rel(la, lb):.3e}, grad rel {_rel(grad_a, grad_b):.3e}')
        assert _rel(la, lb) <= 1e-5, (name, float(la), float(lb))
        assert float(grad_b.abs().max()) > 0 and _rel(grad_a, grad_b) <= 1e-5, (name, _rel(grad_a, grad_b))


def test_graph_replay_of_diffaug_steps_matches_eager_with_changing_draws():
    from rick_amd.synth import synth_reals, synth_tensor
    size, B = 32, 2
    real = [synth_reals(B, size=size, seed=470 + k).cuda() for k in range(6)]
    lat = {k: synth_tensor(f'daug/lat/{k}', (B if k != 'plr' else 1, 8, 512)).cuda() for k in ('d', 'g', 'plr')}
    pl_noise = synth_tensor('daug/pl', (1, 3, size, size)).cuda()

    def run(graphs):
        tr = _trainer(size, B)
        noises = [getattr(tr.g.noises, f'noise_{i}') for i in range(tr.g.num_layers)]
        tr.enable_graphs(graphs)
        tr._draw_inject('d')
        tr._draw_inject = lambda key: None
        tr._graph_latents = lambda key, batch: lat[key]
        static_real = torch.empty_like(real[0])
        losses = []
        for k in range(6):
            static_real.copy_(real[k])
            tr.d_step(static_real, None, g_noise=noises, graph=True)
            tr.r1_step(static_real, graph=True)
            tr.g_step(None, g_noise=noises, graph=True)
            tr.plr_step(None, pl_noise=pl_noise, g_noise=noises, graph=True)
            tr.ema_step()
            losses.append(torch.stack([tr.losses[n].clone() for n in ('d', 'r1', 'g', 'path')]))
        torch.cuda.synchronize()
        if graphs:
            assert all('graphs' in tr._gs[k] for k in ('d', 'r1', 'g'))       # replayed, not re-captured eagerly
        return tr, torch.stack(losses)
    eager, le = run(False)
    graph, lg = run(True)
    assert eager.diffaug_source.k == graph.diffaug_source.k == 24
    torch.testing.assert_close(lg, le, rtol=1e-5, atol=1e-6)
    for fa, fb in ((eager.g_flat, graph.g_flat), (eager.d_flat, graph.d_flat)):
        torch.testing.assert_close(fb.flat, fa.flat, rtol=1e-5, atol=1e-6)


def test_diffaug_off_leaves_the_trainer_as_it_was():
    """diffaug='' is the default: step outputs are bit-identical to a trainer whose config never touched the field, and no
    DiffAugment state appears."""
    from rick_amd.synth import synth_latents, synth_reals
    from rick_amd.train import RickTrainer, TrainConfig
    from tests.test_gpu_models import build
    size, B = 32, 2
    z, real = synth_latents(B, seed=71).cuda(), synth_reals(B, size=size, seed=72).cuda()

    def run(**kw):
        g, d = build(size)
        tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, **kw), g, d, *build(size))
        noises = [getattr(tr.g.noises, f'noise_{i}') for i in range(tr.g.num_layers)]
        out = [tr.d_step(real, [z], g_noise=noises).clone(), tr.r1_step(real).clone(), tr.g_step([z], g_noise=noises).clone()]
        assert tr._augmenter is None            # no policy, and with it no parameter block of any step
        return tr, out
    (a, la), (b, lb) = run(), run(diffaug='')
    assert all(torch.equal(x, y) for x, y in zip(la, lb))
    for fa, fb in ((a.g_flat, b.g_flat), (a.d_flat, b.d_flat)):
        assert torch.equal(fa.flat, fb.flat) and torch.equal(fa.grad, fb.grad)
