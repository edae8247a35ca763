"""Adaptive discriminator augmentation on the GPU (rick_amd/csrc/augment.hip):

  1. per-call times of the fused op against the composed path (reflect pad -> upfirdn2d -> grid_sample -> upfirdn2d -> crop ->
     colour) at 256 px, batch 4 and 8, forward and forward + backward;
  2. steady-state graph-mode images/s of the full iteration mix (D every iteration, R1 every 16th, G, path length every 4th, EMA)
     at 256 px, batch 4, with augmentation off, at fixed p = 0.5 and adaptive, alternated in one process.

  python tools/bench_augment.py [--iters 64] [--rounds 3]"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rick_amd import augment as A  # noqa: E402


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def per_call(size=256, reps=50):
    for B in (4, 8):
        torch.manual_seed(0)
        x = (torch.rand(B, 3, size, size, device='cuda') * 2 - 1).requires_grad_(True)
        G, pads = A.draw_affine(0.5, B, size, size)
        C = A.sample_color(0.5, B)
        prm = A.upload_params(A.aug_params(G, C, size, size, pads), 'cuda')
        gy = torch.randn(B, 3, size, size, device='cuda')
        fused_f = lambda: A.augment_fused(x.detach(), prm)                                       # noqa: E731
        comp_f = lambda: A.apply_color(A.random_apply_affine(x.detach(), 0.5, G)[0], C)         # noqa: E731
        fused_b = lambda: torch.autograd.grad(A.augment_fused(x, prm), x, gy)                    # noqa: E731
        comp_b = lambda: torch.autograd.grad(A.apply_color(A.random_apply_affine(x, 0.5, G)[0], C), x, gy)   # noqa: E731
        print(f'per call {size} px batch {B} pads {pads}: forward fused {timed(fused_f, reps):.3f} ms, composed {timed(comp_f, reps):.3f} ms; '
              f'forward+backward fused {timed(fused_b, reps):.3f} ms, composed {timed(comp_b, reps):.3f} ms', flush=True)


def iteration_mix(iters, rounds, size=256, B=4):
    from rick_amd.models import Discriminator, Generator
    from rick_amd.synth import synth_reals
    from rick_amd.train import RickTrainer, TrainConfig
    modes = {'off': dict(augment=False), 'p=0.5': dict(augment=True, augment_p=0.5), 'adaptive': dict(augment=True, augment_p=0.0)}
    trainers = {}
    for name, kw in modes.items():
        torch.manual_seed(1)
        g, d = Generator(size, 512, 8).cuda(), Discriminator(size).cuda()
        tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, **kw), g, d, Generator(size, 512, 8).cuda(),
                         Discriminator(size).cuda())
        tr.enable_graphs(True)
        if name == 'adaptive':
            tr.ada_p = 0.5                                      # start where the fixed run sits; the controller moves it
        trainers[name] = (tr, synth_reals(B, size, seed=2).cuda())
        tr.prepare_graphs(trainers[name][1])
    res = {k: [] for k in modes}
    for r in range(rounds):
        for name, (tr, real) in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(iters):
                tr.iteration(16 * 64 + r * iters + i, real)
            torch.cuda.synchronize()
            res[name].append(B * iters / (time.perf_counter() - t0))
    for name in modes:
        v = sorted(res[name])
        print(f'iteration mix {size} px batch {B} graphs, augment {name}: {v[len(v) // 2]:.1f} images/s (rounds {", ".join(f"{x:.1f}" for x in res[name])})'
              + (f', p now {trainers[name][0].ada_p:.4f}' if name == 'adaptive' else ''), flush=True)
    off = sorted(res['off'])[rounds // 2]
    print(f'ratio p=0.5 / off: {sorted(res["p=0.5"])[rounds // 2] / off:.3f}; adaptive / off: {sorted(res["adaptive"])[rounds // 2] / off:.3f}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    a = ap.parse_args()
    per_call()
    iteration_mix(a.iters, a.rounds)
