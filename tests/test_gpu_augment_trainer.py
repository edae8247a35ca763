"""The trainer with adaptive discriminator augmentation (TrainConfig.augment): an eager augmented iteration against the same
iteration built from the composed augment.py path, graph replay against eager with changing transforms and p, the checkpoint key."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Source:
    """Pinned transforms for RickTrainer.aug_source: call k draws (G, C) from seed 1000 + k at the trainer's current p."""

    def __init__(self, tr):
        self.tr, self.k, self.log = tr, 0, []

    def __call__(self, n):
        from rick_amd.augment import draw_affine, sample_color
        size = self.tr.cfg.size
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(1000 + self.k)
            G, _ = draw_affine(self.tr.ada_p, n, size, size)          # (with the reflect-pad retry loop)
            C = sample_color(self.tr.ada_p, n)
        self.k += 1
        self.log.append((G, C))
        return G, C


def _trainer(size, B, **kw):
    from rick_amd.train import RickTrainer, TrainConfig
    from tests.test_gpu_models import build
    g, d = build(size)
    tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, augment=True, **kw), g, d, *build(size))
    tr.aug_source = _Source(tr)
    return tr


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def test_eager_augmented_steps_match_the_composed_path(monkeypatch):
    """One augmented iteration (D on cat(augment(fake), augment(real)), R1 on the augmented reals, G through the augmentation)
    equals the same iteration of the same trainer with the composed augment.py path (float64 on the host, rounded to fp32 once)
    in place of the fused op, for the same transforms: losses and flat gradients of every step to 1e-5."""
    import rick_amd.train as T
    from rick_amd.augment import apply_color, random_apply_affine
    from rick_amd.synth import synth_latents, synth_reals, synth_tensor
    size, B = 32, 2
    z, real = synth_latents(B, seed=31).cuda(), synth_reals(B, size=size, seed=32).cuda()

    def composed_for(src):
        """augment_fused's stand-in: the composed path with the transforms the trainer's source drew for this step"""
        def comp(t, GC):
            return apply_color(random_apply_affine(t.double().cpu(), 0.8, GC[0])[0], GC[1]).float().to(t.device)

        def op(x, params):
            if x.shape[0] == 2 * B:                   # D step: cat(fake, real), drawn real first
                real_gc, fake_gc = src.log[-2:]
                return torch.cat([comp(x[:B], fake_gc), comp(x[B:], real_gc)])
            return comp(x, src.log[-1])
        return op

    def run(with_composed):
        tr = _trainer(size, B, augment_p=0.8)
        if with_composed:
            monkeypatch.setattr(T, 'augment_fused', composed_for(tr.aug_source))
        noises = [synth_tensor(f'augnoise/{i}', tuple(getattr(tr.g.noises, f'noise_{i}').shape)).cuda() for i in range(tr.g.num_layers)]
        out = []
        for step in (lambda: tr.d_step(real, [z], g_noise=noises), lambda: tr.r1_step(tr._aug_real),
                     lambda: tr.g_step([z], g_noise=noises)):
            loss = step().clone()
            out.append((loss, tr.d_flat.grad.clone(), tr.g_flat.grad.clone()))
        monkeypatch.undo()
        return tr, out
    fused, a = run(False)
    comp_tr, b = run(True)
    assert len(fused.aug_source.log) == 3 and all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
                                                  for x, y in zip(fused.aug_source.log, comp_tr.aug_source.log))
    for name, (la, da, ga), (lb, db, gb) in zip(('d', 'r1', 'g'), a, b):
        assert _rel(la, lb) <= 1e-5, (name, float(la), float(lb))
        grad_a, grad_b = (ga, gb) if name == 'g' else (da, db)
        assert float(grad_b.abs().max()) > 0 and _rel(grad_a, grad_b) <= 1e-5, (name, _rel(grad_a, grad_b))


def test_graph_replay_of_augmented_steps_matches_eager_with_changing_transforms_and_p():
    from rick_amd.synth import synth_reals, synth_tensor
    size, B = 32, 2
    real = [synth_reals(B, size=size, seed=370 + k).cuda() for k in range(6)]
    lat = {k: synth_tensor(f'aug/lat/{k}', (B if k != 'plr' else 1, 8, 512)).cuda() for k in ('d', 'g', 'plr')}
    pl_noise = synth_tensor('aug/pl', (1, 3, size, size)).cuda()
    ps = [0.2, 0.5, 0.9, 1.0, 0.35, 0.7]

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
            tr.ada_p = ps[k]
            static_real.copy_(real[k])
            tr.d_step(static_real, None, g_noise=noises, graph=True)
            tr.r1_step(tr._aug_real, graph=True)
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
    assert eager.aug_source.k == graph.aug_source.k == 18
    torch.testing.assert_close(lg, le, rtol=1e-5, atol=1e-6)
    for fa, fb in ((eager.g_flat, graph.g_flat), (eager.d_flat, graph.d_flat)):
        torch.testing.assert_close(fb.flat, fa.flat, rtol=1e-5, atol=1e-6)


def _reference_ada(steps, target, length, p0):
    """train_dynamic_update_prune.py:440-459 transcribed; steps: one (sum of signs of D's real logits, global batch) per D step."""
    ada_aug_p, ada_aug_step, acc, out = p0, target / length, [0.0, 0], []
    for sgn, n in steps:
        acc = [acc[0] + sgn, acc[1] + n]
        if acc[1] > 255:
            pred_signs, n_pred = acc
            ada_aug_p += (1 if pred_signs / n_pred > target else -1) * ada_aug_step * n_pred
            ada_aug_p = min(1, max(0, ada_aug_p))
            acc = [0.0, 0]
        out.append(ada_aug_p)
    return out


def _log_real_logits(tr, B):
    """Copy D's real logits of every D step (the second half of its cat(fake, real) pass) into a static buffer: a forward hook
    that also runs inside a graph capture, so replays refill the buffer too."""
    buf = torch.zeros(B, 1, device='cuda')

    def hook(_m, _inp, out):
        if out[0].shape[0] == 2 * B:
            buf.copy_(out[0][B:])
    tr.d.register_forward_hook(hook)
    return buf


@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'graphs'])
def test_adaptive_p_follows_the_reference_over_the_sign_of_real_logits(graphs):
    """Adaptive p through the trainer: D's real-logit signs summed on the device, read once n > 255 (here after 64 D steps of
    4 images), p moved, the sum zeroed — the same trajectory as the reference fed the same logits.  The logits of each step are
    re-evaluated outside the trainer: D before the step on the step's augmented reals (one call: its minibatch statistics are
    those of the real half of the trainer's cat(fake, real) pass)."""
    from rick_amd.synth import synth_reals
    from tests.test_gpu_models import build
    size, B, length = 32, 4, 2_000
    tr = _trainer(size, B, augment_p=0.0, ada_length=length)
    tr.enable_graphs(graphs)
    tr.ada_p = 0.5
    _, d_ref = build(size)
    static_real = torch.empty(B, 3, size, size, device='cuda')
    steps, ps, sums = [], [], []
    for k in range(140):
        static_real.copy_(synth_reals(B, size=size, seed=500 + k % 7).cuda())
        d_ref.load_state_dict(tr.d.state_dict())
        tr.d_step(static_real, None, graph=True)
        with torch.no_grad():
            steps.append((float(torch.sign(d_ref(tr._aug_real)[0]).sum()), B))
        ps.append(tr.ada_p)
        sums.append(float(tr._ada_sum))
    if graphs:
        assert 'graphs' in tr._gs['d']
    want = _reference_ada(steps, 0.6, length, 0.5)
    assert ps == pytest.approx(want, abs=1e-12)
    assert ps[62] == 0.5 and ps[63] != 0.5 and ps[127] != ps[126]       # updated after image 256 and 512, not before
    # between updates the device sum holds exactly the signs since the last update; it restarts at zero after one
    assert sums[62] == sum(sg for sg, _ in steps[:63]) and sums[63] == 0 and sums[64] == steps[64][0]


def test_augmentation_off_leaves_the_trainer_as_it_was():
    """augment=False: the augment flags change nothing — bit-identical weights and losses to a default TrainConfig over eager and
    graph-replayed iterations, no augmentation state, and the D step's loss is D's loss on the plain cat(fake, real)."""
    from rick_amd.synth import synth_latents, synth_reals, synth_tensor
    from rick_amd.train import RickTrainer, TrainConfig, d_logistic_loss
    from tests.test_gpu_models import build
    size, B = 32, 2
    real = [synth_reals(B, size=size, seed=600 + k).cuda() for k in range(5)]
    lat = {k: synth_tensor(f'augoff/lat/{k}', (B if k != 'plr' else 1, 8, 512)).cuda() for k in ('d', 'g', 'plr')}
    pl_noise = synth_tensor('augoff/pl', (1, 3, size, size)).cuda()
    z = synth_latents(B, seed=61).cuda()

    def run(**kw):
        g, d = build(size)
        tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, **kw), g, d, *build(size))
        noises = [getattr(tr.g.noises, f'noise_{i}') for i in range(tr.g.num_layers)]
        state = {k: v.detach().clone() for k, v in tr.d.state_dict().items()}
        with torch.no_grad():
            fake, _ = tr.g([z], noise=noises)
        first = tr.d_step(real[0], [z], g_noise=noises).clone()           # eager
        _, d_ref = build(size)
        d_ref.load_state_dict(state)
        with torch.no_grad():
            fp, rp = d_ref(torch.cat([fake, real[0]]), calls=2)[0].chunk(2)
        torch.testing.assert_close(first, d_logistic_loss(rp, fp), rtol=1e-5, atol=0)      # (no_grad forward: same kernels)
        tr.enable_graphs(True)
        tr._draw_inject('d')
        tr._draw_inject = lambda key: None
        tr._graph_latents = lambda key, batch: lat[key]
        static_real = torch.empty_like(real[0])
        for k in range(5):
            static_real.copy_(real[k])
            tr.d_step(static_real, None, g_noise=noises, graph=True)
            tr.r1_step(static_real, graph=True)
            tr.g_step(None, g_noise=noises, graph=True)
            tr.plr_step(None, pl_noise=pl_noise, g_noise=noises, graph=True)
            tr.ema_step()
        torch.cuda.synchronize()
        assert tr._augmenter is None and tr._ada_sum is None and getattr(tr, '_aug_real', None) is None
        return tr
    a, b = run(), run(augment_p=0.7, ada_target=0.2, ada_length=10)
    for fa, fb in ((a.g_flat, b.g_flat), (a.d_flat, b.d_flat), (a.g_ema_flat, b.g_ema_flat), (a.d_ema_flat, b.d_ema_flat)):
        assert torch.equal(fa.flat, fb.flat)
    for k in ('d', 'r1', 'g', 'path'):
        assert torch.equal(a.losses[k], b.losses[k])


def test_checkpoint_keeps_ada_p_only_when_augmenting():
    from rick_amd import checkpoint
    tr = _trainer(32, 2)
    tr.ada_p = 0.4375
    sd = checkpoint.state_dict(tr)
    assert sd['ada_aug_p'] == 0.4375
    tr.ada_p = 0.0
    checkpoint.resume(tr, sd)
    assert tr.ada_p == 0.4375
    fixed = _trainer(32, 2, augment_p=0.25)           # a fixed p is configuration: a checkpoint's p does not override it
    checkpoint.resume(fixed, sd)
    assert fixed.ada_p == 0.25
    from rick_amd.train import RickTrainer, TrainConfig
    from tests.test_gpu_models import build
    g, d = build(32)
    plain = RickTrainer(TrainConfig(size=32, batch=2, warmup_iter=0), g, d, *build(32))
    assert 'ada_aug_p' not in checkpoint.state_dict(plain)
    checkpoint.resume(plain, sd)
    assert plain.ada_p == 0.0


def _ada_dp_worker(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK='0', HSA_ENABLE_IPC_MODE_LEGACY='0')
    from rick_amd.dist import DataParallelGrads, init_from_env
    from rick_amd.synth import synth_reals
    init_from_env('gloo')
    torch.cuda.set_device(0)
    size, B = 32, 2
    torch.manual_seed(rank)                         # each rank draws its own samples' transforms from its own host RNG
    from rick_amd.train import RickTrainer, TrainConfig
    from tests.test_gpu_models import build
    g, d = build(size)
    tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, augment=True, ada_length=2_000), g, d, *build(size),
                     dp=DataParallelGrads(bucket_bytes=256 * 1024))
    tr.ada_p = 0.5
    buf = _log_real_logits(tr, B)
    signs, ps = [], []
    for k in range(70):                               # 4 global images per step: the first update after step 64
        tr.d_step(synth_reals(B, size=size, seed=700 + 10 * rank + k % 5).cuda(), [torch.randn(B, 512, device='cuda')])
        signs.append(float(torch.sign(buf).sum()))
        ps.append(tr.ada_p)
    torch.cuda.synchronize()
    q.put((rank, signs, ps))
    torch.distributed.destroy_process_group()


def test_two_ranks_hold_the_same_adaptive_p_from_the_global_sign_statistic():
    """World-2 gloo on one GPU: the sign sums of both ranks are summed at the update, so both ranks hold the same p, equal to the
    reference controller (single-process DataParallel over the global batch) fed the concatenated signs."""
    import socket

    import torch.multiprocessing as mp
    from tests.test_gpu_dp import _get
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_ada_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    outs = sorted([_get(q, procs, 600) for _ in procs], key=lambda o: o[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, s0, p0), (_, s1, p1) = outs
    assert p0 == p1
    want = _reference_ada([(a + b, 4) for a, b in zip(s0, s1)], 0.6, 2_000, 0.5)
    assert p0 == pytest.approx(want, abs=1e-12)
    assert p0[62] == 0.5 and p0[63] != 0.5                  # the update happened, after image 256 of the global batch
