"""The elastic-weight-consolidation pass (rick_amd/ewc.py, rick_amd/csrc/ewc.hip) on the GPU: the two launches of ``penalty_`` at the
size of the 256-px generator's optimised slice, and the trainer's G step at 256 px, batch 4, with the term on and off.

  python tools/bench_ewc.py [--iters 200] [--rounds 5] [--skip-step]
  rocprofv3 --kernel-trace --stats ... -- python tools/bench_ewc.py --trace --iters 100            (kernel times, a run of its own)

The pass is timed by device events around back-to-back CALLS of ``ewc.accumulate_`` (Python wrapper and both launches included)
after a warm-up call, with and without a mask, the variants taking turns inside each of `rounds` windows; median and range over the
windows are printed.  Calls rotate over two sets of the four streams (0.38 GB per set), more than the 256 MiB the chip can keep
between two uses of a line.  GB/s counts the bytes the algorithm needs — 20 B per element, 21 with a mask — over the call time: a
call-level figure.  The kernel's own share of the 8 TB/s peak needs kernel time: --trace runs nothing but the pass, for a
kernel-trace run.  The G step is timed the same way, eager and as a replayed step graph, the trainers with and without the term
taking turns.  Prints a readable report and one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_GBS = 8000.0


def timed(fns, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        fns[k % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / iters


def alternated(variants, iters, rounds):
    """variants: {name: [fn, ...]} -> {name: (median, min, max)} seconds per call over `rounds` windows, the variants taking turns
    inside every round (drift of the clock or a neighbour's load hits all of them alike)."""
    for fns in variants.values():
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fns in variants.items():
            times[k].append(timed(fns, max(len(fns), iters)))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def slice_size(size=256):
    """Elements of the optimised slice of the generator's FlatParams (padding included): computed from the model, on the CPU."""
    from rick_amd.models import Generator
    from rick_amd.train import FlatParams, g_optim_filter
    flat = FlatParams(Generator(size, 512, 8, channel_multiplier=2).named_parameters(), g_optim_filter)
    return flat.hi - flat.lo


def streams(n, sets=2):
    gen = torch.Generator('cuda').manual_seed(0)
    out = []
    for _ in range(sets):
        anchor = torch.randn(n, device='cuda', generator=gen)
        theta = anchor + 1e-2 * torch.randn(n, device='cuda', generator=gen)
        fisher = 1e-2 * torch.rand(n, device='cuda', generator=gen)
        out.append((theta, anchor, fisher, torch.randn(n, device='cuda', generator=gen)))
    return out


def pass_report(args, n):
    from rick_amd._lib import lib
    from rick_amd.ewc import accumulate_
    sets = streams(n)
    mask = torch.zeros(n, dtype=torch.uint8, device='cuda')
    partials = torch.empty(lib.rick_ewc_blocks(n), dtype=torch.float64, device='cuda')
    out = torch.zeros((), dtype=torch.float64, device='cuda')
    t = alternated({'no_mask': [(lambda s=s: accumulate_(*s, 5.0, partials=partials, out=out)) for s in sets],
                    'mask': [(lambda s=s: accumulate_(*s, 5.0, mask=mask, partials=partials, out=out)) for s in sets]},
                   args.iters, args.rounds)
    res = {'elements': n, 'blocks': int(lib.rick_ewc_blocks(n))}
    print(f'the pass at n = {n} ({n * 4 / 1e6:.1f} MB per stream, {lib.rick_ewc_blocks(n)} blocks): us per CALL (wrapper + both '
          f'launches), median of {args.rounds} alternated windows [min-max]; GB/s = bytes needed over the median call time')
    for name, per in (('no_mask', 20), ('mask', 21)):
        med, lo, hi = t[name]
        gbs = per * n / med / 1e9
        res[f'pass_{name}_us'] = [v * 1e6 for v in t[name]]
        res[f'pass_{name}_call_gbs'] = gbs
        res[f'pass_{name}_call_bandwidth_over_peak'] = gbs / PEAK_GBS
        print(f'  {name:8s} {med * 1e6:8.1f} us [{lo * 1e6:.1f}-{hi * 1e6:.1f}]  {gbs:6.0f} GB/s  {gbs / PEAK_GBS:.2f} of the '
              f'{PEAK_GBS / 1e3:.0f} TB/s peak (call-level)', flush=True)
    return res


def trace(args, n):
    """What a `rocprofv3 --kernel-trace --stats` run wraps: nothing but the pass, so that the averages of ewc_kernel<false>,
    ewc_kernel<true> and ewc_finish_kernel in the trace are the kernel times at this size."""
    from rick_amd._lib import lib
    from rick_amd.ewc import accumulate_
    sets = streams(n)
    mask = torch.zeros(n, dtype=torch.uint8, device='cuda')
    partials = torch.empty(lib.rick_ewc_blocks(n), dtype=torch.float64, device='cuda')
    for k in range(args.iters):
        accumulate_(*sets[k % 2], 5.0, partials=partials)
        accumulate_(*sets[k % 2], 5.0, mask=mask, partials=partials)
    torch.cuda.synchronize()
    print(f'trace: {args.iters} x (pass without a mask, pass with one) at n = {n}: {20 * n / 1e6:.1f} / {21 * n / 1e6:.1f} MB needed per '
          f'call; share of peak = that over (kernel time x {PEAK_GBS / 1e3:.0f} TB/s)')


def step_report(args):
    from rick_amd.models import Discriminator, Generator
    from rick_amd.synth import synth_state_dict
    from rick_amd.train import RickTrainer, TrainConfig
    from tests.shapes import discriminator_shapes, generator_shapes
    size, B = 256, 4
    sg, sd = synth_state_dict(generator_shapes(size)), synth_state_dict(discriminator_shapes(size))

    def make():
        g, d = Generator(size, 512, 8, channel_multiplier=2), Discriminator(size)
        g.load_state_dict(sg, strict=False)
        d.load_state_dict(sd, strict=False)
        return g.cuda(), d.cuda()
    res = {}
    for graphs in (False, True):
        trainers = {}
        for name, weight in (('off', 0.0), ('on', 5.0)):
            g, d = make()
            g_ema, d_ema = make()
            state = {k: v.detach().clone() + 1e-2 for k, v in g.state_dict().items()}
            tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, ewc_weight=weight), g, d, g_ema, d_ema,
                             ewc=(state, None) if weight else None)
            if graphs:
                tr.enable_graphs(True)
                for _ in range(3):                             # two eager warm-up steps and the capture
                    tr.g_step(None, graph=True)
            trainers[name] = tr
        z = [torch.randn(B, 512, device='cuda')]
        t = alternated({k: [(lambda tr=tr: tr.g_step(None, graph=True)) if graphs else (lambda tr=tr: tr.g_step(z))]
                        for k, tr in trainers.items()}, max(10, args.iters // 10), args.rounds)
        mode = 'graph' if graphs else 'eager'
        for name in ('off', 'on'):
            res[f'g_step_{mode}_ms_ewc_{name}'] = [v * 1e3 for v in t[name]]
            print(f'g_step at 256 px, batch {B}, {mode}, term {name}: {t[name][0] * 1e3:.3f} ms [{t[name][1] * 1e3:.3f}-'
                  f'{t[name][2] * 1e3:.3f}]', flush=True)
        res[f'g_step_{mode}_ms_added'] = (t['on'][0] - t['off'][0]) * 1e3
        del trainers
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--elements', type=int, default=0, help='size of the pass (default: the 256-px generator\'s optimised slice)')
    args = ap.parse_args()
    n = args.elements or slice_size()
    if not torch.cuda.is_available():
        raise SystemExit(f'tools/bench_ewc.py needs an MI355X (the pass would run over n = {n} elements)')
    if args.trace:
        return trace(args, n)
    res = {'metric': 'ewc_pass', 'size': 256, 'batch': 4}
    res.update(pass_report(args, n))
    torch.cuda.empty_cache()
    if not args.skip_step:
        res.update(step_report(args))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
