"""DiffAugment on the GPU (rick_amd/csrc/diffaug.hip):

  1. per-call times at N = 8, 256 x 256, policy color,translation,cutout: the fused forward, the fused forward + adjoint, and the
     published composition in torch ops on the device (its draws on the device, as published), forward and forward + backward;
  2. steady-state graph-mode images/s of the full iteration mix (D every iteration, R1 every 16th, G, path length every 4th, EMA)
     at 256 px, batch 4, with DiffAugment off and on, alternated in one process.

  python tools/bench_diffaug.py [--reps 200] [--iters 64] [--rounds 3] [--no-mix]"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rick_amd import diffaug as DA  # noqa: E402

POLICY = 'color,translation,cutout'


def composed_device(x):
    """The seven published steps in torch ops, everything (draws included) on x's device."""
    n, _, h, w = x.shape
    dev = x.device
    x = x + (torch.rand(n, 1, 1, 1, dtype=x.dtype, device=dev) - 0.5)
    mean = x.mean(dim=1, keepdim=True)
    x = (x - mean) * (torch.rand(n, 1, 1, 1, dtype=x.dtype, device=dev) * 2) + mean
    mean = x.mean(dim=[1, 2, 3], keepdim=True)
    x = (x - mean) * (torch.rand(n, 1, 1, 1, dtype=x.dtype, device=dev) + 0.5) + mean
    sr, sc = DA.shift_range(h), DA.shift_range(w)
    tr = torch.randint(-sr, sr + 1, size=[n, 1, 1], device=dev)
    tc = torch.randint(-sc, sc + 1, size=[n, 1, 1], device=dev)
    gb, gr, gc = torch.meshgrid(torch.arange(n, device=dev), torch.arange(h, device=dev), torch.arange(w, device=dev), indexing='ij')
    gr = torch.clamp(gr + tr + 1, 0, h + 1)
    gc = torch.clamp(gc + tc + 1, 0, w + 1)
    x = F.pad(x, [1, 1, 1, 1, 0, 0, 0, 0]).permute(0, 2, 3, 1).contiguous()[gb, gr, gc].permute(0, 3, 1, 2)
    ch, cw = DA.cut_size(h), DA.cut_size(w)
    orow = torch.randint(0, h + (1 - ch % 2), size=[n, 1, 1], device=dev)
    ocol = torch.randint(0, w + (1 - cw % 2), size=[n, 1, 1], device=dev)
    gb, gr, gc = torch.meshgrid(torch.arange(n, device=dev), torch.arange(ch, device=dev), torch.arange(cw, device=dev), indexing='ij')
    gr = torch.clamp(gr + orow - ch // 2, min=0, max=h - 1)
    gc = torch.clamp(gc + ocol - cw // 2, min=0, max=w - 1)
    mask = torch.ones(n, h, w, dtype=x.dtype, device=dev)
    mask[gb, gr, gc] = 0
    return x * mask.unsqueeze(1)


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def per_call(reps, n=8, size=256):
    torch.manual_seed(0)
    x = (torch.rand(n, 3, size, size, device='cuda') * 2 - 1).requires_grad_(True)
    gy = torch.randn(n, 3, size, size, device='cuda')
    prm = DA.upload_params(DA.check_params(DA.draw_params(n, size, size, POLICY), size, size), 'cuda')
    fns = {'fused forward': lambda: DA.diffaug_fused(x.detach(), prm),
           'fused forward + adjoint': lambda: torch.autograd.grad(DA.diffaug_fused(x, prm), x, gy),
           'composed forward': lambda: composed_device(x.detach()),
           'composed forward + backward': lambda: torch.autograd.grad(composed_device(x), x, gy)}
    res = {k: [] for k in fns}
    for _ in range(3):                                     # alternated: three rounds of each, the median is reported
        for k, fn in fns.items():
            res[k].append(timed(fn, reps))
    for k, v in res.items():
        print(f'per call N={n} {size}x{size} {POLICY}: {k}: {sorted(v)[1]:.4f} ms (rounds {", ".join(f"{t:.4f}" for t in v)})', flush=True)
    moved = 2 * 3 * (n * 3 * size * size * 4)               # each direction: the batch read twice (sum, apply) and written once
    pair = sorted(res['fused forward + adjoint'])[1]
    print(f'fused pair: {moved / 1e6:.1f} MB moved by the algorithm, {moved / pair / 1e6:.1f} GB/s over the call time (launch overhead '
          f'included); fused pair / composed pair = {pair / sorted(res["composed forward + backward"])[1]:.3f}', flush=True)


def iteration_mix(iters, rounds, size=256, B=4):
    from rick_amd.models import Discriminator, Generator
    from rick_amd.synth import synth_reals
    from rick_amd.train import RickTrainer, TrainConfig
    modes = {'off': dict(), 'on': dict(diffaug=POLICY)}
    trainers = {}
    for name, kw in modes.items():
        torch.manual_seed(1)
        g, d = Generator(size, 512, 8).cuda(), Discriminator(size).cuda()
        tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, **kw), g, d, Generator(size, 512, 8).cuda(),
                         Discriminator(size).cuda())
        tr.enable_graphs(True)
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
        print(f'iteration mix {size} px batch {B} graphs, diffaug {name}: {v[len(v) // 2]:.1f} images/s (rounds '
              f'{", ".join(f"{x:.1f}" for x in res[name])})', flush=True)
    print(f'ratio on / off: {sorted(res["on"])[rounds // 2] / sorted(res["off"])[rounds // 2]:.3f}')


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--iters', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-mix', action='store_true')
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_diffaug.py needs an MI355X')
    per_call(a.reps)
    if not a.no_mix:
        iteration_mix(a.iters, a.rounds)
