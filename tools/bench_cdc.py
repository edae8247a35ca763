"""The distance-consistency loss (rick_amd/cdc.py) on the GPU: rick_gram_f32 and rick_rowmix_f32 at the 13 feature shapes of the
256-px generator at batch 4, next to ``X.flatten(1) @ X.flatten(1).t()`` in fp32 and to the customary B (B - 1) loop of
F.cosine_similarity on the same tensors; then the trainer's G step at 256 px, batch 4, with the loss on and off.

  python tools/bench_cdc.py [--iters 200] [--rounds 5] [--skip-step]
  rocprofv3 --kernel-trace --stats ... -- python tools/bench_cdc.py --trace-large --iters 50      (kernel times, a run of its own)

Times are device events around back-to-back CALLS (Python wrapper, workspace allocation and launches included), after a warm-up
call: per layer the four variants take turns inside each of `rounds` windows, and the median and the range over the windows are
printed.  Each call of a rotation takes the next of several copies of the features, enough copies to exceed the 256 MiB the chip
can keep between two uses of a line (at most 16: the small layers stay cache-resident and are launch-bound either way).  GB/s
counts the rows read once (gram) and read plus written once (rowmix): the bytes the algorithm needs, not the bytes a kernel
moved, over the call time — a call-level figure.  A kernel's share of peak needs kernel time: --trace-large runs only gram and
rowmix at the largest feature shape, for a kernel-trace run.  Prints a readable report and one JSON line."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_GBS = 8000.0


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
    """variants: {name: (fns, weight)} -> {name: (median, min, max)} seconds per call over `rounds` windows, the variants taking
    turns inside every round (so that drift of the clock or a neighbour's load hits all of them alike); weight scales a
    variant's calls per window."""
    for fns, _ in variants.values():
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (fns, weight) in variants.items():
            times[k].append(timed(fns, max(len(fns), int(iters * weight))))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in times.items()}


def cosine_loop(x):
    B = x.shape[0]
    return [F.cosine_similarity(x[i].reshape(1, -1), x[j].reshape(1, -1)) for i in range(B) for j in range(B) if j != i]


def kernels_report(args, feats):
    from rick_amd import cdc
    dev = feats[0].device
    rows_out, res = [], {}
    print('us per CALL (Python wrapper + workspace allocation + launches), median of %d alternated windows [min-max]; GB/s = rows '
          'read once (gram) / read + written once (rowmix) over the median call time' % args.rounds)
    print(f'{"layer":>5} {"shape":>20} {"MB":>7} | {"gram us":>22} {"GB/s":>6} | {"rowmix us":>22} {"GB/s":>6} | {"X@X.t us":>22} | '
          f'{"cos loop us":>24}')

    def cell(t):
        return f'{t[0] * 1e6:8.1f} [{t[1] * 1e6:.1f}-{t[2] * 1e6:.1f}]'
    for l, f in enumerate(feats):
        B, by = f.shape[0], f.numel() * 4
        copies = max(1, min(16, -(-600 * 2 ** 20 // by)))
        xs = [f.clone() if k else f for k in range(copies)]
        assert all(cdc._sample_dense(x) for x in xs)
        rws = [cdc._rows(x) for x in xs]
        outs = [torch.empty_like(r) for r in rws[:2]]
        A = torch.randn(B, B, device=dev)
        iters = args.iters if by < 32 * 2 ** 20 else max(20, args.iters // 4)
        with torch.no_grad():
            t = alternated({
                'gram': ([(lambda x=x: cdc.gram(x)) for x in xs], 1.0),
                'rowmix': ([(lambda k=k, r=r: cdc.rowmix(A, r, out=outs[k % 2])) for k, r in enumerate(rws)], 1.0),
                'matmul': ([(lambda x=x: x.flatten(1) @ x.flatten(1).t()) for x in xs], 0.5),
                'loop': ([(lambda x=x: cosine_loop(x)) for x in xs], 0.1)}, iters, args.rounds)
        gb_gram, gb_mix = by / t['gram'][0] / 1e9, 2 * by / t['rowmix'][0] / 1e9
        rows_out.append(dict(layer=l, shape=list(f.shape), mbytes=by / 1e6, gram_us=[v * 1e6 for v in t['gram']], gram_call_gbs=gb_gram,
                             rowmix_us=[v * 1e6 for v in t['rowmix']], rowmix_call_gbs=gb_mix,
                             matmul_us=[v * 1e6 for v in t['matmul']], cosine_loop_us=[v * 1e6 for v in t['loop']]))
        print(f'{l:5d} {str(tuple(f.shape)):>20} {by / 1e6:7.2f} | {cell(t["gram"]):>22} {gb_gram:6.0f} | {cell(t["rowmix"]):>22} '
              f'{gb_mix:6.0f} | {cell(t["matmul"]):>22} | {cell(t["loop"]):>24}', flush=True)
        del xs, rws, outs
        torch.cuda.empty_cache()
    big = [r for r in rows_out if r['mbytes'] > 100]
    if big:
        res['gram_call_bandwidth_over_peak_large'] = min(r['gram_call_gbs'] for r in big) / PEAK_GBS
        res['rowmix_call_bandwidth_over_peak_large'] = min(r['rowmix_call_gbs'] for r in big) / PEAK_GBS
        print(f'large layers (> 100 MB), call-level bandwidth over the {PEAK_GBS / 1e3:.0f} TB/s peak (NOT a kernel\'s share of peak: '
              f'kernel times come from a rocprofv3 --kernel-trace run of --trace-large): gram '
              f'{res["gram_call_bandwidth_over_peak_large"]:.2f}, rowmix {res["rowmix_call_bandwidth_over_peak_large"]:.2f}')
    res['layers'] = rows_out
    return res


def trace_large(args):
    """What a `rocprofv3 --kernel-trace --stats` run wraps: nothing but gram and rowmix on the 256-px generator's largest feature
    shape (4 x 128 x 256 x 256 channels-last, 134 MB, five rotating copies), so that the per-kernel averages of gram_kernel<4, true>,
    gram_finish_kernel and rowmix_kernel<4, true> in the trace are the kernel times at that shape."""
    from rick_amd import cdc
    gen = torch.Generator('cuda').manual_seed(0)
    xs = [(torch.randn(4, 128, 256, 256, device='cuda', generator=gen) + 1).contiguous(memory_format=torch.channels_last)
          for _ in range(5)]
    out, A = torch.empty_like(cdc._rows(xs[0])), torch.randn(4, 4, device='cuda', generator=gen)
    with torch.no_grad():
        for k in range(args.iters):
            cdc.gram(xs[k % 5])
            cdc.rowmix(A, cdc._rows(xs[k % 5]), out=out)
    torch.cuda.synchronize()
    print(f'trace-large: {args.iters} x (gram, rowmix) on 4 x 128 x 256 x 256, 134.2 MB of rows per call')


def step_report(args, make):
    from rick_amd.train import RickTrainer, TrainConfig
    res = {}
    B = 4
    for name, weight in (('off', 0.0), ('on', 1000.0)):
        g, d = make()
        g_ema, d_ema = make()
        src = make()[0]
        tr = RickTrainer(TrainConfig(size=256, batch=B, warmup_iter=0, cdc_weight=weight, cdc_batch=4), g, d, g_ema, d_ema,
                         g_source=src)
        z = [torch.randn(B, 512, device='cuda')]
        t = alternated({'step': ([lambda: tr.g_step(z)], 1.0)}, max(10, args.iters // 10), args.rounds)['step']
        res[f'g_step_eager_ms_cdc_{name}'] = [v * 1e3 for v in t]
        print(f'g_step at 256 px, batch {B}, eager, loss {name}: {t[0] * 1e3:.3f} ms [{t[1] * 1e3:.3f}-{t[2] * 1e3:.3f}]', flush=True)
        del tr, g, d, g_ema, d_ema, src
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--trace-large', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_cdc.py needs an MI355X')
    torch.backends.cuda.matmul.allow_tf32 = False
    if args.trace_large:
        return trace_large(args)
    from rick_amd.models import Discriminator, Generator
    from rick_amd.synth import synth_state_dict
    from tests.shapes import discriminator_shapes, generator_shapes
    size = 256
    sg, sd = synth_state_dict(generator_shapes(size)), synth_state_dict(discriminator_shapes(size))

    def make():
        g, d = Generator(size, 512, 8, channel_multiplier=2), Discriminator(size)
        g.load_state_dict(sg, strict=False)
        d.load_state_dict(sd, strict=False)
        return g.cuda(), d.cuda()
    g, _ = make()
    with torch.no_grad():
        _, feats = g([torch.randn(4, 512, device='cuda', generator=torch.Generator('cuda').manual_seed(0))], return_feats=True)
    feats = [f.detach() for f in feats]
    del g
    res = {'metric': 'cdc_gram_rowmix', 'batch': 4, 'size': size}
    res.update(kernels_report(args, feats))
    del feats
    torch.cuda.empty_cache()
    if not args.skip_step:
        res.update(step_report(args, make))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
