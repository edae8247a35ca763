"""LPIPS (rick_amd/lpips.py) on the GPU: VGG16-trunk throughput of the HIP path against the same network as a torch fp32
composition (F.conv2d ... on the same device), the pair kernel's time and achieved read bandwidth, and the wall time of
intra_lpips at the reference's defaults (1 000 samples at 256^2, 10 centres, 50 per cluster) with generator sampling
timed separately, plus its peak device memory.  Seeded synthetic weights (timing only).

  python tools/bench_lpips.py [--iters 10] [--skip-eval]
  python tools/bench_lpips.py --backward [--iters 10] [--project-steps 1000]
--backward measures the differentiable path instead (LPIPS.loss): at 256^2 and n = 1 and 25 the features forward alone and
forward + loss + backward with respect to the image, and the wall time of a projection of one 256-px image
(rick_amd/project.py) next to its generator part and its LPIPS part, each timed alone over the same number of steps.
Prints a readable report and one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def trunk_flops(size=256):
    """Algorithmic FLOPs (2 x multiply-adds) of the 13 convolutions for one image; pools and norms not counted."""
    from rick_amd.lpips import STAGES
    total, h = 0, size
    for s, stage in enumerate(STAGES):
        if s:
            h //= 2
        for _, ci, co in stage:
            total += 2 * 9 * ci * co * h * h
    return total


def pair_bytes(na, nb, size=256):
    """Bytes the pair kernel reads: every A image once per 16-wide B tile and vice versa (taps + inverse norms)."""
    from rick_amd.lpips import CHANNELS, _tap_hw
    per_image = sum(h * w * (c + 1) * 4 for (h, w), c in zip(_tap_hw(size, size), CHANNELS))
    return per_image * (na * -(-nb // 16) + nb * -(-na // 16))


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


def backward_report(args):
    from rick_amd.lpips import LPIPS
    from tests.lpips_f64 import synthetic_state_dict
    dev, size = 'cuda', 256
    sd = synthetic_state_dict(0)
    flops = trunk_flops(size)
    res = {'metric': 'lpips_vgg16_backward', 'gflop_per_image_forward': flops / 1e9}
    for n in (1, 25):
        net = LPIPS.load(sd, device=dev, batch=n)
        x = torch.rand(n, 3, size, size, device=dev, generator=torch.Generator(dev).manual_seed(n)) * 2 - 1
        tf = net.features(torch.rand(n, 3, size, size, device=dev, generator=torch.Generator(dev).manual_seed(100 + n)) * 2 - 1)
        out = net.new_features(n)
        xr = x.clone().requires_grad_(True)

        def fwd_bwd():
            return torch.autograd.grad(net.loss(xr, tf).sum(), xr)
        t_f = timed(lambda: net.features(x, out=out), args.iters)
        t_fb = timed(fwd_bwd, args.iters)
        res.update({f'forward_ms_n{n}': t_f * 1e3, f'forward_backward_ms_n{n}': t_fb * 1e3, f'ratio_n{n}': t_fb / t_f,
                    f'forward_tflops_n{n}': flops * n / t_f / 1e12})
        print(f'N={n:3d}: features forward {t_f * 1e3:8.3f} ms ({flops * n / t_f / 1e12:5.1f} TFLOP/s)   forward + loss + backward '
              f'{t_fb * 1e3:8.3f} ms   x{t_fb / t_f:.2f}', flush=True)
        del net, tf, out
        torch.cuda.empty_cache()
    if args.project_steps > 0:
        from rick_amd.models import Generator
        from rick_amd.project import project
        from rick_amd.synth import synth_state_dict
        from tests.shapes import generator_shapes
        steps = args.project_steps
        g = Generator(size, 512, 8, channel_multiplier=2)
        g.load_state_dict(synth_state_dict(generator_shapes(size)), strict=False)
        g = g.to(dev).requires_grad_(False)
        net = LPIPS.load(sd, device=dev, batch=1)
        with torch.no_grad():
            target = g([torch.randn(1, 512, device=dev, generator=torch.Generator(dev).manual_seed(5))], randomize_noise=False)[0]
        project(g, target, net, steps=5, rng=torch.Generator().manual_seed(0))          # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, losses = project(g, target, net, steps=steps, rng=torch.Generator().manual_seed(0))
        torch.cuda.synchronize()
        t_total = time.perf_counter() - t0
        w = g.mean_latent(1000).detach().requires_grad_(True)
        go = torch.randn(1, 3, size, size, device=dev)

        def g_step():
            img, _ = g([w + 0.0], input_is_latent=True, randomize_noise=False)
            return torch.autograd.grad(img, w, go)
        xr = target.clone().requires_grad_(True)
        tf = net.features(target.flip(-1))
        t_g = timed(g_step, min(steps, 50))
        t_l = timed(lambda: torch.autograd.grad(net.loss(xr, tf).sum(), xr), min(steps, 50))
        res.update({'project_steps': steps, 'project_total_s': t_total, 'project_generator_s': t_g * steps,
                    'project_lpips_s': t_l * steps, 'project_loss_first': float(losses[0]), 'project_loss_last': float(losses[-1])})
        print(f'projection of one {size}-px image, {steps} steps: {t_total:.2f} s; alone, the generator forward + backward is '
              f'{t_g * steps:.2f} s and the LPIPS forward + backward {t_l * steps:.2f} s; loss {float(losses[0]):.4f} -> '
              f'{float(losses[-1]):.4f}', flush=True)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--skip-eval', action='store_true')
    ap.add_argument('--backward', action='store_true')
    ap.add_argument('--project-steps', type=int, default=1000)
    args = ap.parse_args()
    if args.backward:
        torch.backends.cudnn.allow_tf32 = False
        torch.backends.cuda.matmul.allow_tf32 = False
        return backward_report(args)
    from rick_amd.lpips import LPIPS, _cpu_taps, scale_input
    from tests.lpips_f64 import synthetic_state_dict
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev, size = 'cuda', 256
    sd = synthetic_state_dict(0)
    net = LPIPS.load(sd, device=dev, batch=50)
    convs = {k: (w.to(dev), b.to(dev)) for k, (w, b) in net.convs.items()}
    flops = trunk_flops(size)
    res = {'metric': 'lpips_vgg16', 'gflop_per_image': flops / 1e9}
    feats = {}
    for n in (25, 50):
        x = torch.rand(n, 3, size, size, device=dev, generator=torch.Generator(dev).manual_seed(n)) * 2 - 1
        out = net.new_features(n)
        with torch.no_grad():
            t_hip = timed(lambda: net.features(x, out=out), args.iters)
            t_torch = timed(lambda: _cpu_taps(convs, scale_input(x)[0]), max(2, args.iters // 2))
            ref = _cpu_taps(convs, scale_input(x)[0])[-1].permute(0, 2, 3, 1)
            d = float((out.taps[-1] - ref).abs().max() / ref.abs().max())
        feats[n] = out
        res.update({f'hip_img_s_n{n}': n / t_hip, f'torch_fp32_img_s_n{n}': n / t_torch, f'hip_tflops_n{n}': flops * n / t_hip / 1e12,
                    f'torch_tflops_n{n}': flops * n / t_torch / 1e12, f'speedup_n{n}': t_torch / t_hip,
                    f'max_rel_diff_relu5_3_vs_torch_n{n}': d})
        print(f'trunk N={n:3d}: HIP {n / t_hip:7.1f} img/s ({flops * n / t_hip / 1e12:6.1f} TFLOP/s)   torch fp32 '
              f'{n / t_torch:7.1f} img/s ({flops * n / t_torch / 1e12:6.1f} TFLOP/s)   x{t_torch / t_hip:.2f}   '
              f'relu5_3 max rel diff {d:.2e}', flush=True)
    for na, nb in ((25, 10), (50, 50)):
        fa, fb = feats[50].narrow(0, na), (feats[25].narrow(0, nb))
        t = timed(lambda: net.distances(fa, fb), args.iters)
        by = pair_bytes(na, nb, size)
        res[f'pair_ms_{na}x{nb}'] = t * 1e3
        res[f'pair_gbs_{na}x{nb}'] = by / t / 1e9
        print(f'pairs {na} x {nb}: {t * 1e3:.3f} ms, {by / 1e9:.2f} GB of feature tiles read, {by / t / 1e9:.0f} GB/s', flush=True)
    del feats, net
    torch.cuda.empty_cache()
    if not args.skip_eval:
        from rick_amd.evaluate import intra_lpips, sample_images
        from rick_amd.models import Generator
        from rick_amd.synth import synth_state_dict
        from tests.shapes import generator_shapes
        g = Generator(size, 512, 8, channel_multiplier=2)
        g.load_state_dict(synth_state_dict(generator_shapes(size)), strict=False)
        g = g.to(dev)
        imgs, _ = sample_images(g, 10, n_sample_store=10, generator=torch.Generator(dev).manual_seed(1))
        centers = ((imgs / 2 + 0.5) * 255 + 0.5).clamp(0, 255).to(torch.uint8)        # 10 samples as the centres
        sample_images(g, 50)                                               # warm-up
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        net = LPIPS.load(sd, device=dev, batch=25)
        intra_lpips(g, centers, net, n_samples=50, cluster_size=50)        # warm-up (allocator, kernels)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        val, per, counts = intra_lpips(g, centers, net, rng=torch.Generator().manual_seed(0))
        torch.cuda.synchronize()
        t_total = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated() - base
        t0 = time.perf_counter()
        sample_images(g, 1000, n_sample_store=25)
        torch.cuda.synchronize()
        t_g = time.perf_counter() - t0
        res.update({'intra_lpips_total_s': t_total, 'intra_lpips_g_sampling_s': t_g, 'intra_lpips_peak_gib': peak / 2**30,
                    'intra_lpips_value': val, 'intra_lpips_counts': counts.tolist()})
        print(f'intra_lpips, 1000 samples at {size}^2, 10 centres, 50 per cluster: {t_total:.2f} s (G sampling alone '
              f'{t_g:.2f} s); peak memory {peak / 2**30:.2f} GiB above the generator; value {val:.4f}, '
              f'counts {counts.tolist()}', flush=True)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
