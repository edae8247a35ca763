"""DINOv2 features (rick_amd/dinov2.py) on the GPU: synthetic ViT-S/14, ViT-B/14 and ViT-L/14 weights at 224^2 (257 tokens),
n = 25 from 256^2 inputs.  Reports images/s beside the same computation as an fp32 torch composition on the GPU
(rick_amd.dinov2.torch_forward, the module's CPU-path code, on device tensors), and in the same run the time of the fc1 GEMMs
of one forward pass with the GELU epilogue (rick_inc_conv_vit_f32) against rick_inc_conv_lin_f32 with QuickGELU on the identical
shape, operands and buffers: what the erf costs in the epilogue.  Seeded synthetic weights (timing only).

  python tools/bench_dinov2.py [--iters 20] [--rounds 5] [--models S B L]

The implementations are timed alternately, `--rounds` times each after a warm-up of both; the report gives the median and
every round.  Prints a readable report and one JSON line; profiles/dinov2_bench.txt is a run's output."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODELS = {'S': (dict(width=384, patch=14, image=224, layers=12, mlp=1536), 6),
          'B': (dict(width=768, patch=14, image=224, layers=12, mlp=3072), 12),
          'L': (dict(width=1024, patch=14, image=224, layers=24, mlp=4096), 16)}


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


def median(v):
    return sorted(v)[len(v) // 2]


def fc1_pair(net, n):
    """(the fc1 launches of one forward pass of n images, the same GEMMs on rick_inc_conv_lin_f32 with QuickGELU)."""
    from rick_amd.cliptower import issue, linear
    tf, c = net._plan.tf, net.cfg
    gelu = [s for s in tf.launches(n) if s.what == 'fc']
    quick = [linear('fc', op['fc'], n * c.tokens, c.width, c.mlp, tf.ln, tf.hid, act=1) for op in tf.gemm]
    assert len(gelu) == len(quick) == c.layers and all(s.name == 'rick_inc_conv_vit_f32' for s in gelu)
    return (lambda: issue(gelu)), (lambda: issue(quick))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20, help='passes per timed round')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--models', nargs='+', default=list(MODELS), choices=list(MODELS))
    args = ap.parse_args()
    from rick_amd.dinov2 import Dinov2Features, params_from_state_dict, torch_forward
    from tests.dinov2_f64 import synthetic_dinov2_state_dict
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev, px, n = 'cuda', 256, 25
    res = {'metric': 'dinov2_vit14_224'}
    for name in args.models:
        cfg_, heads = MODELS[name]
        net = Dinov2Features(params_from_state_dict(synthetic_dinov2_state_dict(cfg_, 0)), device=dev, batch=n, size=224, heads=heads)
        cfg = net.cfg
        pd = {k: v.to(dev) for k, v in net.params.items()}
        x = torch.rand(n, 3, px, px, device=dev, generator=torch.Generator(dev).manual_seed(n)) * 2 - 1
        hip = lambda: net(x)                                                  # noqa: E731
        with torch.no_grad():
            ref = lambda: torch_forward(pd, cfg, x)                           # noqa: E731
            diff = float((hip() - ref()).abs().max() / ref().abs().max())
            timed(hip, 3), timed(ref, 3)                                      # warm-up of both
            th, tt = [], []
            for _ in range(args.rounds):
                th.append(timed(hip, args.iters))
                tt.append(timed(ref, args.iters))
        h, t = median(th), median(tt)
        print(f'ViT-{name}/14 at 224, n={n} from {px}^2: HIP kernels {n / h:8.1f} img/s ({h * 1e3:.2f} ms)   torch fp32 composition '
              f'{n / t:8.1f} img/s ({t * 1e3:.2f} ms)   hip / torch = {h / t:.3f}   max rel diff {diff:.2e}')
        print('    rounds (ms)  hip: ' + ' '.join(f'{v * 1e3:.2f}' for v in th) + '   torch: ' + ' '.join(f'{v * 1e3:.2f}' for v in tt))
        gelu, quick = fc1_pair(net, n)
        timed(gelu, 3), timed(quick, 3)
        tg, tq = [], []
        for _ in range(args.rounds):
            tg.append(timed(gelu, args.iters))
            tq.append(timed(quick, args.iters))
        g, q = median(tg), median(tq)
        print(f'    fc1 GEMMs of one pass ({cfg.layers} x [{n * cfg.tokens}, {cfg.width}] -> {cfg.mlp}): GELU epilogue {g * 1e3:.3f} ms   '
              f'QuickGELU epilogue {q * 1e3:.3f} ms   gelu / quickgelu = {g / q:.3f}')
        print('    rounds (ms)  gelu: ' + ' '.join(f'{v * 1e3:.3f}' for v in tg) + '   quickgelu: ' + ' '.join(f'{v * 1e3:.3f}' for v in tq),
              flush=True)
        res.update({f'hip_img_s_{name}': n / h, f'torch_img_s_{name}': n / t, f'hip_ms_{name}': h * 1e3, f'torch_ms_{name}': t * 1e3,
                    f'max_rel_diff_vs_torch_{name}': diff, f'fc1_gelu_ms_{name}': g * 1e3, f'fc1_quickgelu_ms_{name}': q * 1e3,
                    f'fc1_gelu_over_quickgelu_{name}': g / q})
        del net, pd
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
