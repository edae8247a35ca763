"""Perceptual path length (rick_amd/ppl.py) on the GPU: the latents kernel, the paired LPIPS kernel against the route it replaces
(all pairs + diagonal) on the same features, the metric end to end in both spaces, and the error ratios that
tests/test_gpu_ppl.py bounds.  Seeded synthetic weights.

  python tools/bench_ppl.py [--iters 20] [--rounds 5] [--samples 200] [--skip-errors] [--out profiles/ppl_bench.txt]

Times are device events around `iters` calls after a warm-up call of the same shape; the two distance routes alternate for
`rounds` rounds in one process and the report gives the median and the range over the rounds.  Bytes are the taps and inverse
norms each route has to read, computed from the shapes.  The report goes to stdout and to --out, and ends in one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / iters


def image_bytes(size):
    from rick_amd.lpips import CHANNELS, _tap_hw
    return sum(h * w * (c + 1) * 4 for (h, w), c in zip(_tap_hw(size, size), CHANNELS))


def med(xs):
    return f'{statistics.median(xs) * 1e3:.3f} ms (range {min(xs) * 1e3:.3f} .. {max(xs) * 1e3:.3f})'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--samples', type=int, default=200)
    ap.add_argument('--skip-errors', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ppl_bench.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ppl.py measures on the GPU; none is visible')
    from rick_amd.lpips import LPIPS
    from rick_amd.models import Generator
    from rick_amd.ppl import path_latents, perceptual_path_length
    from rick_amd.synth import synth_state_dict
    from tests import ppl_f64
    from tests.lpips_f64 import synthetic_state_dict
    from tests.shapes import generator_shapes
    dev, size, n = 'cuda', 256, 25
    lines, res = [], {'metric': 'ppl'}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f'# tools/bench_ppl.py --iters {args.iters} --rounds {args.rounds} --samples {args.samples}   '
        f'({torch.cuda.get_device_name(0)}, torch {torch.__version__})')
    # ---- the latents kernel
    gen = torch.Generator(dev).manual_seed(0)
    a, b = torch.randn(n, 512, device=dev, generator=gen), torch.randn(n, 512, device=dev, generator=gen)
    t = torch.rand(n, device=dev, generator=gen)
    for space in ('w', 'z'):
        ts = [timed(lambda: path_latents(a, b, t, 1e-4, space), 50 * args.iters) for _ in range(args.rounds)]
        res[f'latents_us_{space}'] = statistics.median(ts) * 1e6
        say(f'path_latents, {n} paths x 512, space {space}: {statistics.median(ts) * 1e6:.1f} us per call, launch included '
            f'(range {min(ts) * 1e6:.1f} .. {max(ts) * 1e6:.1f})')
    # ---- paired against all pairs + diagonal, same features
    sd = synthetic_state_dict(0)
    net = LPIPS.load(sd, device=dev, batch=2 * n)
    x = torch.rand(2 * n, 3, size, size, device=dev, generator=gen) * 2 - 1
    inter = net.features(x, out=net.new_features(2 * n))
    fa, fb = net.features(x[0::2].contiguous(), out=net.new_features(n)), net.features(x[1::2].contiguous(), out=net.new_features(n))
    routes = {'all_pairs_diagonal': lambda: torch.diagonal(net.distances(fa, fb)).contiguous(),
              'paired': lambda: net.paired(fa, fb), 'paired_interleaved': lambda: net.paired(inter)}
    same = torch.equal(routes['paired'](), routes['all_pairs_diagonal']()) and torch.equal(routes['paired_interleaved'](), routes['paired']())
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(timed(fn, args.iters))
    per = image_bytes(size)
    read = {'all_pairs_diagonal': per * 2 * n * -(-n // 16), 'paired': per * 2 * n, 'paired_interleaved': per * 2 * n}
    say(f'{n} paired LPIPS distances at {size}^2 from stored features (results bit-identical across the routes: {same}):')
    for k in routes:
        m = statistics.median(times[k])
        res[f'{k}_ms'] = m * 1e3
        say(f'  {k:20s} {med(times[k])}   reads {read[k] / 1e9:.2f} GB -> {read[k] / m / 1e9:.0f} GB/s')
    res['paired_speedup'] = res['all_pairs_diagonal_ms'] / res['paired_ms']
    res['bit_identical'] = same
    say(f'  paired is x{res["paired_speedup"]:.2f} the all-pairs route (medians)')
    del net, inter, fa, fb, x
    torch.cuda.empty_cache()
    # ---- end to end
    g = Generator(size, 512, 8, channel_multiplier=2)
    g.load_state_dict(synth_state_dict(generator_shapes(size)), strict=False)
    g = g.to(dev).eval()
    net = LPIPS.load(sd, device=dev, batch=2 * n)
    for space in ('w', 'z'):
        perceptual_path_length(g, net, n_samples=2 * n, space=space)                # warm-up, same batch shape
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ppl, _ = perceptual_path_length(g, net, n_samples=args.samples, space=space)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res[f'pairs_per_s_{space}'] = args.samples / dt
        say(f'perceptual_path_length, {size} px generator, space {space}, {args.samples} paths in batches of {n} (eps 1e-4, noise '
            f'drawn on the device): {dt:.2f} s, {args.samples / dt:.1f} pairs/s (value {ppl:.4g}; synthetic weights)')
    del g, net
    torch.cuda.empty_cache()
    # ---- the error ratios of tests/test_gpu_ppl.py
    if not args.skip_errors:
        S, N, eps = 32, 6, 1e-2
        sg, sl = synth_state_dict(generator_shapes(S, n_mlp=2, cm=1)), synthetic_state_dict(3)
        g = Generator(S, 512, 2, channel_multiplier=1)
        g.load_state_dict(sg, strict=False)
        g = g.to(dev).eval()
        net = LPIPS.load(sl, device=dev, batch=8, size=S)
        latents, noise = ppl_f64.pinned_paths(N, S, 11)
        say(f'error against the fp64 restatement (tests/ppl_f64.py), {S} px generator, {N} pinned paths, eps {eps:g}: max relative '
            f'error of the per-path distances, the CPU fp32 composition\'s own, and their ratio (bounded by 8 in tests/test_gpu_ppl.py)')
        for space in ('w', 'z'):
            for crop in (False, True):
                ref = ppl_f64.path_distances(sg, sl, S, *latents, noise, eps, space, crop)
                f32 = ppl_f64.path_distances(sg, sl, S, *latents, noise, eps, space, crop, dtype=torch.float32)
                yard = float(((f32.double() - ref).abs() / ref).max())
                _, d = perceptual_path_length(g, net, n_samples=N, batch=4, eps=eps, space=space, sampling='full', crop=crop,
                                              latents=latents, noise=noise)
                err = float(((d.double().cpu() - ref).abs() / ref).max())
                res[f'err_ratio_{space}_{"crop" if crop else "full"}'] = err / yard
                say(f'  space {space} crop {str(crop):5s}: device {err:.2e}   fp32 composition {yard:.2e}   ratio {err / yard:.2f}')
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
