"""The patch-level discriminator head (rick_amd/patchd.py) on the GPU: ``patch_head`` forward plus backward at the two production
maps, (4, 512, 32, 32) and (4, 512, 16, 16), on the kernels of rick_amd/csrc/patchd.hip and on the composition of the existing
ops (``patchd.use_kernels(False)``: op.conv2d + fused_leaky_relu, what ran a one-channel 3x3 convolution before the kernels
existed, plus the seven small torch launches of the composition's fp64 bias join); then the
trainer's eager D and G steps at 256 px, batch 4: image-level, and patch-level at each of the three taps.

  python tools/bench_patchd.py [--iters 200] [--rounds 5] [--skip-step]
  rocprofv3 --kernel-trace --stats ... -- python tools/bench_patchd.py --trace --iters 50        (kernel times, a run of its own)
  rocprofv3 --kernel-trace --stats ... -- python tools/bench_patchd.py --trace --composed --iters 50        (the composition's launches)

Times are device events around back-to-back CALLS (Python wrapper, autograd, workspace allocation and launches included), after
a warm-up call: the variants take turns inside each of `rounds` windows, and the median and the range over the windows are
printed.  Each call of a rotation takes the next of 64 copies of the feature map (537 MB of them at the larger shape; the head is
expected to be launch-bound either way).  --trace runs one path alone (the kernels, or with --composed the composition) at both
shapes, for a kernel-trace run.  Prints a readable report and one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [(4, 512, 32, 32), (4, 512, 16, 16)]


def timed(fns, iters):
    """Seconds per call of fns[k % len(fns)](), one event-timed window (the caller has warmed the functions up)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(iters):
        fns[k % len(fns)]()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / iters


def alternated(variants, iters, rounds):
    """variants: {name: fns} -> {name: (median, min, max)} seconds per call over `rounds` windows, the variants taking turns
    inside every round (so that drift of the clock or a neighbour's load hits all of them alike)."""
    for fns in variants.values():
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fns in variants.items():
            times[k].append(timed(fns, max(len(fns), iters)))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def _operands(shape, copies):
    N, C, H, W = shape
    gen = torch.Generator('cuda').manual_seed(sum(shape))
    xs = [torch.randn(N, C, H, W, device='cuda', generator=gen).contiguous(memory_format=torch.channels_last).requires_grad_(True)
          for _ in range(copies)]
    w = torch.randn(1, C, 3, 3, device='cuda', generator=gen).requires_grad_(True)
    b = torch.full((1,), 0.1, device='cuda').requires_grad_(True)
    g = torch.randn(N, 1, H, W, device='cuda', generator=gen)
    return xs, w, b, g, 1.0 / (9 * C) ** 0.5


def _fwd_bwd(x, w, b, g, wscale):
    from rick_amd import patchd
    out = patchd.patch_head(x, w, b, wscale)
    return torch.autograd.grad(out, (x, w, b), g)


def _switched(on, fn):
    from rick_amd import patchd

    def run():
        prev = patchd.use_kernels(on)
        try:
            return fn()
        finally:
            patchd.use_kernels(prev)
    return run


def head_report(args):
    res = {}
    print('patch_head forward + backward (gX, gw, gb), us per CALL, median of %d alternated windows [min-max]' % args.rounds)
    for shape in SHAPES:
        by = 4 * shape[0] * shape[1] * shape[2] * shape[3]
        xs, w, b, g, wscale = _operands(shape, max(16, min(64, 512 * 2 ** 20 // by)))
        t = alternated({'kernels': [_switched(True, lambda x=x: _fwd_bwd(x, w, b, g, wscale)) for x in xs],
                        'composed': [_switched(False, lambda x=x: _fwd_bwd(x, w, b, g, wscale)) for x in xs]}, args.iters, args.rounds)
        tag = 'x'.join(map(str, shape))
        for k, v in t.items():
            res[f'head_{k}_us_{tag}'] = [u * 1e6 for u in v]
        print(f'  {tag:>14} ({by / 1e6:.1f} MB): kernels {t["kernels"][0] * 1e6:7.1f} [{t["kernels"][1] * 1e6:.1f}-{t["kernels"][2] * 1e6:.1f}]'
              f'   composed {t["composed"][0] * 1e6:7.1f} [{t["composed"][1] * 1e6:.1f}-{t["composed"][2] * 1e6:.1f}]'
              f'   ratio {t["composed"][0] / t["kernels"][0]:.2f}', flush=True)
        del xs
        torch.cuda.empty_cache()
    return res


def trace(args):
    """What a `rocprofv3 --kernel-trace --stats` run wraps: one path alone, forward + backward, at both shapes."""
    from rick_amd import patchd
    patchd.use_kernels(not args.composed)
    for shape in SHAPES:
        xs, w, b, g, wscale = _operands(shape, 16)
        for k in range(args.iters):
            _fwd_bwd(xs[k % 16], w, b, g, wscale)
        torch.cuda.synchronize()
        print(f'trace: {args.iters} x patch_head forward + backward on {shape}, {"composed" if args.composed else "kernels"}')


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
    real = torch.randn(B, 3, size, size, device='cuda').clamp_(-1, 1)
    z = [torch.randn(B, 512, device='cuda')]
    for name, freq in (('feature_off', 0), ('feature_on', 4)):
        g, d = make()
        g_ema, d_ema = make()
        tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, subspace_freq=freq), g, d, g_ema, d_ema)
        variants = {'d_image': [lambda: tr.d_step(real, z)], 'g_image': [lambda: tr.g_step(z)]}
        if freq:
            for p in range(3):
                variants[f'd_patch{p}'] = [lambda p=p: tr.d_step(real, z, patch=p)]
                variants[f'g_patch{p}'] = [lambda p=p: tr.g_step(z, patch=p)]
        t = alternated(variants, max(10, args.iters // 10), args.rounds)
        for k, v in t.items():
            res[f'{k}_eager_ms_{name}'] = [u * 1e3 for u in v]
            print(f'  {name} {k:>9} at 256 px, batch {B}, eager: {v[0] * 1e3:.3f} ms [{v[1] * 1e3:.3f}-{v[2] * 1e3:.3f}]', flush=True)
        del tr, g, d, g_ema, d_ema
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--trace', action='store_true')
    ap.add_argument('--composed', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_patchd.py needs an MI355X')
    if args.trace:
        return trace(args)
    res = {'metric': 'patch_head', 'batch': 4}
    res.update(head_report(args))
    if not args.skip_step:
        res.update(step_report(args))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
