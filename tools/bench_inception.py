"""InceptionV3 feature extractor (rick_amd/inception.py) on the GPU: throughput of the HIP path against the same network as a
torch fp32 composition (F.conv2d ... on the same device), and the wall time of a 5 000-image FID evaluation
(Evaluator.compute_inception_score) split into G sampling, features and statistics.  Seeded random weights (timing only).

  python tools/bench_inception.py [--iters 10] [--nsamples 5000] [--size 256]
  python tools/bench_inception.py --score [--iters 10] [--nsamples 5000] [--size 256]
--score: the Inception Score path instead (InceptionV3Logits, rick_amd.evaluate.InceptionScoreStats): img/s of the logits
network at the native size and resized to 299, the head's share of it (fc + softmax rows + accumulation), and the wall time of
a 5 000-sample Evaluator.compute_inception_score(iscore=True).
Prints a readable report and one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def seeded_state_dict(seed=0):
    from rick_amd.inception import units
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, ci, co, (kh, kw), _, _ in units():
        sd[f'{name}.conv.weight'] = torch.randn(co, ci, kh, kw, generator=g) / (ci * kh * kw) ** 0.5
        sd[f'{name}.bn.weight'] = torch.rand(co, generator=g) + 0.5
        sd[f'{name}.bn.bias'] = torch.rand(co, generator=g) * 0.4 - 0.2
        sd[f'{name}.bn.running_mean'] = torch.zeros(co)
        sd[f'{name}.bn.running_var'] = torch.ones(co)
    return sd


def table_flops(size=299):
    """Algorithmic FLOPs (2 x multiply-adds) of the 94 convolutions for one image; pools not counted."""
    from rick_amd.inception import MIXED, STEM0, STEM1, mixed_units
    h = (size - 3) // 2 + 1                               # Conv2d_1a_3x3
    sizes = {'Conv2d_1a_3x3': h}
    h = h - 2
    sizes['Conv2d_2a_3x3'] = h
    sizes['Conv2d_2b_3x3'] = h
    h = (h - 3) // 2 + 1
    sizes['Conv2d_3b_1x1'] = h
    sizes['Conv2d_4a_3x3'] = h - 2
    h = (h - 2 - 3) // 2 + 1
    total = 0
    for name, ci, co, (kh, kw), _, _ in STEM0 + STEM1:
        total += 2 * co * ci * kh * kw * sizes[name] ** 2
    for kind, name, cin, par in MIXED:
        for u in mixed_units(kind, name, cin, par):
            _, ci, co, (kh, kw), (sh, _), (ph, pw) = u
            oh = (h + 2 * ph - kh) // sh + 1
            total += 2 * co * ci * kh * kw * oh * oh
        if kind in ('B', 'D'):
            h = (h - 3) // 2 + 1
    return total


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


def score_mode(args):
    """Throughput of the Inception Score path and the wall time of an evaluation with iscore=True."""
    from rick_amd.evaluate import Evaluator, InceptionScoreStats
    from rick_amd.inception import CLASSES, POOL3, InceptionV3Logits, accumulate_rows, softmax_rows
    dev = 'cuda'
    sd = seeded_state_dict()
    g = torch.Generator().manual_seed(1)
    sd['fc.weight'], sd['fc.bias'] = torch.randn(CLASSES, POOL3, generator=g) * 0.05, torch.randn(CLASSES, generator=g) * 0.1
    res = {'metric': 'inception_score', 'size': args.size}
    nets = {'native': InceptionV3Logits.load(sd, device=dev, batch=100, size=(args.size, args.size)),
            'resize299': InceptionV3Logits.load(sd, device=dev, batch=100, size=None)}
    for tag, net in nets.items():
        for n in (25, 100):
            x = torch.rand(n, 3, args.size, args.size, device=dev, generator=torch.Generator(dev).manual_seed(n)) * 2 - 1
            st = InceptionScoreStats(net, 1 << 40, 1)
            logits = net(x)
            acc = torch.zeros(1, 2 * CLASSES + 1, device=dev, dtype=torch.float64)

            def head():
                net._run_fc(n, logits)
                p, s_, h = softmax_rows(logits)
                accumulate_rows(acc, p, s_, h, 0, 1 << 40)
            t_net = timed(lambda: net(x), args.iters)
            t_all = timed(lambda: st.update(x), args.iters)
            t_head = timed(head, args.iters * 5)
            res[f'{tag}_logits_img_s_n{n}'] = n / t_net
            res[f'{tag}_update_img_s_n{n}'] = n / t_all
            res[f'{tag}_head_share_n{n}'] = t_head / t_all
            print(f'{tag:9s} {args.size}^2 N={n:4d}: logits {n / t_net:8.1f} img/s   update (logits + rows + accumulate) '
                  f'{n / t_all:8.1f} img/s   head (fc + rows + accumulate) {t_head * 1e6:7.1f} us = {100 * t_head / t_all:.2f} % of '
                  f'an update', flush=True)
    if not args.skip_eval:
        from rick_amd.models import Generator
        from rick_amd.synth import synth_state_dict
        from tests.shapes import generator_shapes
        gen = Generator(args.size, 512, 8, channel_multiplier=2)
        gen.load_state_dict(synth_state_dict(generator_shapes(args.size)), strict=False)
        gen = gen.to(dev)
        ns = args.nsamples
        feature_fn = lambda img: img.mean((2, 3))                                 # noqa: E731  (FID is not what is timed here)
        real = torch.randn(ns, 3, device=dev)
        for tag, net in nets.items():
            ev = Evaluator(gen, feature_fn, real, n_sample_store=25, inception_nsamples=100, fid_sample_size=100, is_net=net)
            ev.compute_inception_score(fid=False, iscore=True)                    # warm-up (allocator, kernels)
            ev.inception_nsamples = ev.sample_size = ns
            times = {}
            for iscore in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                score = ev.compute_inception_score(fid=False, iscore=iscore, is_splits=10)
                if iscore:
                    float(score['is'])
                torch.cuda.synchronize()
                times[iscore] = time.perf_counter() - t0
            res[f'eval_{tag}_s'], res[f'eval_{tag}_sampling_only_s'] = times[True], times[False]
            print(f'Evaluator.compute_inception_score(fid=False, iscore=True, is_splits=10), {ns} images at {args.size}^2, '
                  f'{tag}: {times[True]:.2f} s (the same loop without the score: {times[False]:.2f} s)', flush=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--nsamples', type=int, default=5000)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--skip-eval', action='store_true')
    ap.add_argument('--score', action='store_true', help='the Inception Score path instead of the FID features')
    args = ap.parse_args()
    if args.score:
        torch.backends.cudnn.allow_tf32 = False
        torch.backends.cuda.matmul.allow_tf32 = False
        with torch.no_grad():
            score_mode(args)
        return
    from rick_amd.inception import InceptionV3Features, _cpu_forward, fold
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = 'cuda'
    sd = seeded_state_dict()
    net = InceptionV3Features.load(sd, device=dev, dims=2048, batch=100)
    folded = {k: (w.to(dev), b.to(dev)) for k, (w, b) in fold(sd).items()}
    flops = table_flops()
    res = {'metric': 'inception_v3_pool3', 'gflop_per_image': flops / 1e9}
    for n in (25, 100):
        x = torch.rand(n, 3, args.size, args.size, device=dev, generator=torch.Generator(dev).manual_seed(n)) * 2 - 1
        with torch.no_grad():
            t_hip = timed(lambda: net(x), args.iters)
            t_torch = timed(lambda: _cpu_forward(folded, x, 3), max(2, args.iters // 2))
            d = float((net(x) - _cpu_forward(folded, x, 3)).abs().max() / _cpu_forward(folded, x, 3).abs().max())
        res[f'hip_img_s_n{n}'] = n / t_hip
        res[f'torch_fp32_img_s_n{n}'] = n / t_torch
        res[f'hip_tflops_n{n}'] = flops * n / t_hip / 1e12
        res[f'torch_tflops_n{n}'] = flops * n / t_torch / 1e12
        res[f'speedup_n{n}'] = t_torch / t_hip
        res[f'max_rel_diff_vs_torch_n{n}'] = d
        print(f'N={n:4d}: HIP {n / t_hip:8.1f} img/s ({flops * n / t_hip / 1e12:6.1f} TFLOP/s)   torch fp32 '
              f'{n / t_torch:8.1f} img/s ({flops * n / t_torch / 1e12:6.1f} TFLOP/s)   x{t_torch / t_hip:.2f}   '
              f'max rel diff {d:.2e}', flush=True)
    if not args.skip_eval:
        from rick_amd.evaluate import Evaluator, FeatureStats, frechet_distance, sample_images
        from rick_amd.models import Generator
        from rick_amd.synth import synth_state_dict
        from tests.shapes import generator_shapes
        g = Generator(args.size, 512, 8, channel_multiplier=2)
        g.load_state_dict(synth_state_dict(generator_shapes(args.size)), strict=False)
        g = g.to(dev)
        ns = args.nsamples
        real = net(torch.rand(200, 3, args.size, args.size, device=dev) * 2 - 1).repeat(ns // 200 + 1, 1)[:ns]
        ev = Evaluator(g, net, real, n_sample_store=25, inception_nsamples=ns, fid_sample_size=ns)
        ev.inception_nsamples = ev.sample_size = 100                     # warm-up (allocator, kernels)
        ev.compute_inception_score(fid=True)
        ev.inception_nsamples = ev.sample_size = ns
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score = ev.compute_inception_score(fid=True)
        float(score['fid'])
        torch.cuda.synchronize()
        t_total = time.perf_counter() - t0
        t0 = time.perf_counter()
        imgs, _ = sample_images(g, ns, n_sample_store=25)
        torch.cuda.synchronize()
        t_g = time.perf_counter() - t0
        t0 = time.perf_counter()
        feats = torch.cat([net(imgs[i:i + 25]) for i in range(0, ns, 25)])
        torch.cuda.synchronize()
        t_f = time.perf_counter() - t0
        t0 = time.perf_counter()
        fid = frechet_distance(*FeatureStats(2048, dev).update(real).finalize(), *FeatureStats(2048, dev).update(feats).finalize())
        float(fid)
        torch.cuda.synchronize()
        t_s = time.perf_counter() - t0
        res.update({'eval_nsamples': ns, 'eval_total_s': t_total, 'eval_g_sampling_s': t_g, 'eval_features_s': t_f,
                    'eval_statistics_s': t_s})
        print(f'Evaluator.compute_inception_score(fid=True), {ns} images at {args.size}^2: {t_total:.2f} s '
              f'(parts measured separately: G sampling {t_g:.2f} s, features {t_f:.2f} s, statistics {t_s:.2f} s)', flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
