"""VGG16 fc2 features (rick_amd/vgg.py) on the GPU: feature throughput at n = 25 / 100 from 256^2 inputs, the fc kernel alone
on fc1's shape (K = 25088, N = 4096; a 411 MB fp32 weight stream) at M = 25 / 50 against torch's fp32 F.linear on the same
device, and a 5 000-sample Evaluator.compute_inception_score(pr=True) at 256^2 split into G sampling, features and
statistics.  Seeded synthetic weights (timing only).

  python tools/bench_vgg.py [--fc-iters 4000] [--iters 10] [--fc-only] [--skip-eval]
The two fc implementations are timed alternately, `--rounds` times each, after a warm-up of both; a round is `--fc-iters`
launches (a few tenths of a second), and the report gives every round so that the timer's spread is visible.  Successive
launches alternate between two copies of the weights, so no launch finds its 411 MB stream in the 256 MB last-level cache;
the bandwidth figure is weight bytes over kernel time (x, the split-K workspace and the output add under 4 %).  Prints a
readable report and one JSON line."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12            # B/s, MI355X spec


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


def bench_fc(res, iters, rounds):
    from rick_amd import _lib as L
    from rick_amd.vgg import pack_fc_weight
    dev, K, N = 'cuda', 25088, 4096
    g = torch.Generator().manual_seed(0)
    w = torch.randn(N, K, generator=g) * (2.0 / K) ** 0.5
    b = torch.randn(N, generator=g) * 0.02
    wpk, wd, bd = pack_fc_weight(w).to(dev), w.to(dev), b.to(dev)
    wpks, wds = (wpk, wpk.clone()), (wd, wd.clone())              # launches alternate between the two copies
    wbytes = N * K * 4
    for M in (25, 50):
        x = torch.randn(M, K, device=dev, generator=torch.Generator(dev).manual_seed(M))
        ws = torch.empty(L.lib.rick_fc_workspace_floats(M, K, N), device=dev)
        out = torch.empty(M, N, device=dev)

        turn = [0, 0]

        def hip():
            turn[0] ^= 1
            L.check(L.lib.rick_fc_f32(x.data_ptr(), wpks[turn[0]].data_ptr(), bd.data_ptr(), ws.data_ptr(), out.data_ptr(), M, K, N,
                                      1, L.stream_ptr()), 'rick_fc_f32')

        def ref():
            turn[1] ^= 1
            return torch.relu_(F.linear(x, wds[turn[1]], bd))
        hip()
        d = float((out - ref()).abs().max() / ref().abs().max())
        timed(hip, iters), timed(ref, iters)                      # warm-up of both
        th, tt = [], []
        for _ in range(rounds):
            th.append(timed(hip, iters))
            tt.append(timed(ref, iters))
        h, t = sorted(th)[len(th) // 2], sorted(tt)[len(tt) // 2]
        res.update({f'fc1_hip_us_m{M}': h * 1e6, f'fc1_torch_us_m{M}': t * 1e6, f'fc1_hip_hbm_fraction_m{M}': wbytes / h / HBM_PEAK,
                    f'fc1_torch_hbm_fraction_m{M}': wbytes / t / HBM_PEAK, f'fc1_max_rel_diff_vs_torch_m{M}': d})
        print(f'fc1 M={M:2d} (K={K}, N={N}, relu): rick_fc_f32 {h * 1e6:7.1f} us = {wbytes / h / 1e12:.2f} TB/s (weight bytes / time, '
              f'{100 * wbytes / h / HBM_PEAK:.0f} % of the 8 TB/s HBM peak)   torch fp32 F.linear {t * 1e6:7.1f} us = '
              f'{wbytes / t / 1e12:.2f} TB/s ({100 * wbytes / t / HBM_PEAK:.0f} %)   hip / torch = {h / t:.3f}   max rel diff {d:.2e}')
        print('    rounds (us)  hip: ' + ' '.join(f'{v * 1e6:.1f}' for v in th) + '   torch: ' + ' '.join(f'{v * 1e6:.1f}' for v in tt),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--fc-iters', type=int, default=4000, help='launches per timed round of the fc kernel')
    ap.add_argument('--iters', type=int, default=10, help='calls per timing of the whole network')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--fc-only', action='store_true')
    ap.add_argument('--skip-eval', action='store_true')
    args = ap.parse_args()
    from rick_amd.vgg import VGG16Fc2Features
    from tests.vgg_f64 import synthetic_vgg16_state_dict
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev, size = 'cuda', 256
    res = {'metric': 'vgg16_fc2'}
    bench_fc(res, args.fc_iters, args.rounds)
    if args.fc_only:
        print(json.dumps(res))
        return
    sd = synthetic_vgg16_state_dict(0)
    for n, batch in ((25, 25), (100, 50)):
        net = VGG16Fc2Features.load(sd, device=dev, batch=batch)
        x = torch.rand(n, 3, size, size, device=dev, generator=torch.Generator(dev).manual_seed(n)) * 2 - 1
        t = timed(lambda: net(x), args.iters)
        res[f'features_img_s_n{n}'] = n / t
        print(f'features n={n:3d} (batch {batch}) from {size}^2: {n / t:7.1f} img/s ({t * 1e3:.1f} ms)', flush=True)
        del net
        torch.cuda.empty_cache()
    if not args.skip_eval:
        from rick_amd.evaluate import Evaluator, precision_recall_from_features, sample_images
        from rick_amd.models import Generator
        from rick_amd.synth import synth_state_dict
        from tests.shapes import generator_shapes
        n = 5000
        g = Generator(size, 512, 8, channel_multiplier=2)
        g.load_state_dict(synth_state_dict(generator_shapes(size)), strict=False)
        g = g.to(dev)
        net = VGG16Fc2Features.load(sd, device=dev, batch=25)
        pooled = lambda img: F.adaptive_avg_pool2d(img, 4).flatten(1)      # noqa: E731  (FID features are not the subject here)
        real, _ = sample_images(g, 200, n_sample_store=25, generator=torch.Generator(dev).manual_seed(1))
        real_pr = torch.cat([net(real)] * (n // 200))                      # 5 000 real-side rows (timing only)
        real_pr = real_pr + 0.01 * torch.randn(real_pr.shape, device=dev, generator=torch.Generator(dev).manual_seed(2))
        ev = Evaluator(g, pooled, pooled(real), n_sample_store=25, inception_nsamples=n, fid_sample_size=n, pr_feature_fn=net,
                       real_pr_feats=real_pr)
        sample_images(g, 50)                                               # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score = ev.compute_inception_score(fid=False, pr=True)
        p, r = float(score['precision']), float(score['recall'])
        torch.cuda.synchronize()
        t_total = time.perf_counter() - t0
        t0 = time.perf_counter()
        sample_images(g, n, n_sample_store=25)
        torch.cuda.synchronize()
        t_g = time.perf_counter() - t0
        img = real[:25].contiguous()
        t0 = time.perf_counter()
        fake_pr = torch.cat([net(img) for _ in range(n // 25)])
        torch.cuda.synchronize()
        t_f = time.perf_counter() - t0
        t0 = time.perf_counter()
        precision_recall_from_features(real_pr, fake_pr + real_pr * 0.5)
        torch.cuda.synchronize()
        t_s = time.perf_counter() - t0
        res.update({'pr_eval_total_s': t_total, 'pr_eval_g_sampling_s': t_g, 'pr_eval_features_s': t_f, 'pr_eval_statistics_s': t_s,
                    'precision': p, 'recall': r})
        print(f'compute_inception_score(pr=True), {n} samples at {size}^2: {t_total:.2f} s; alone: G sampling {t_g:.2f} s, fc2 '
              f'features {t_f:.2f} s, precision / recall statistics {t_s:.2f} s (precision {p:.3f}, recall {r:.3f}: synthetic '
              f'weights)', flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
