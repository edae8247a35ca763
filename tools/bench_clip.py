"""CLIP image embeddings (rick_amd/clip.py) on the GPU: synthetic ViT-B/32 weights (width 768, 12 layers, 12 heads, MLP 3072,
patch 32, 224^2, projection 512) at n = 25 and n = 100 from 256^2 inputs.  Reports images/s, the device time of every kernel
family (each family's launches of one forward pass, timed alone on the network's own buffers), and in the same run the same
computation as an fp32 torch composition on the GPU (rick_amd.clip.torch_forward, the module's CPU-path code, on device
tensors).  Seeded synthetic weights (timing only).

  python tools/bench_clip.py [--iters 20] [--rounds 5]
  python tools/bench_clip.py --backward      forward + backward of ClipImageFeatures.encode at n = 4, 8 and 25 against the fp32
                                             torch autograd composition on the same GPU, and the backward pass per kernel family
  python tools/bench_clip.py --text          the text tower (rick_amd/cliptext.py): prompts/s for 160 prompts of 77 tokens at the
                                             ViT-B/32 text dimensions (width 512, 8 heads, 12 layers, vocab 49408, random
                                             weights), beside rick_amd.cliptext.torch_text_forward on the same CUDA tensors
The two implementations are timed alternately, `--rounds` times each after a warm-up of both; the report gives the median
and every round.  Prints a readable report and one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VIT_B32 = dict(width=768, patch=32, image=224, layers=12, mlp=3072, dim=512)
VIT_B32_TEXT = dict(width=512, tokens=77, vocab=49408, layers=12, mlp=2048, dim=512)       # 8 heads


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


def pick(launches, *what):
    """A function that issues those of a pass's resolved launches (rick_amd/cliptower.py) whose place in it is one of `what`."""
    from rick_amd.cliptower import issue
    chosen = [s for s in launches if s.what in what]
    assert chosen, what
    return lambda: issue(chosen)


def families(net, n, x):
    """{family: a function that issues that family's launches of one forward pass of n images}, on the plan's buffers."""
    from rick_amd import _lib as L
    plan, c = net._plan, net.cfg
    out = torch.empty(n, c.dim, device=x.device)
    net(x)                                                                    # the launches of n images are resolved
    fwd = plan.fwd[n]
    return {
        'input (bicubic + affine)': lambda: L.check(L.lib.rick_clip_input_f32(x.data_ptr(), plan.x0.data_ptr(), n, x.shape[2], x.shape[3],
                                                                              c.size, L.stream_ptr()), 'rick_clip_input_f32'),
        'patch embedding GEMM': pick(fwd, 'patch'),
        'tokens + ln_pre': pick(fwd, 'tokens'),
        'LayerNorm (2 per layer + ln_post)': pick(fwd, 'ln1', 'ln2', 'ln_post'),
        'q/k/v GEMM': pick(fwd, 'qkv'),
        'attention': pick(fwd, 'attention'),
        'out_proj GEMM + residual': pick(fwd, 'out'),
        'c_fc GEMM + QuickGELU': pick(fwd, 'fc'),
        'c_proj GEMM + residual': pick(fwd, 'proj'),
        'projection (rick_fc_f32)': lambda: plan.tf.project(n, out),
    }


def backward_families(net, n):
    """{family: a function that issues that family's launches of one backward pass of n images}, on the gradient workspace's
    buffers after a differentiable forward run."""
    from rick_amd import _lib as L
    from rick_amd.fc import run_fc
    ws, c = net._grad_workspace(), net.cfg
    bwd = ws.backward_launches(n)
    gx, go = torch.empty(n, 3, 256, 256, device=ws.gt.device), torch.ones(n, c.dim, device=ws.gt.device)
    return {
        'projection^T (rick_fc_f32)': lambda: run_fc(go.data_ptr(), ws.head_t.data_ptr(), ws.head_t_bias.data_ptr(), ws.ws.data_ptr(),
                                                     ws.gpost.data_ptr(), n, c.dim, c.width, 0),
        'LayerNorm backward (2 per layer + ln_post)': pick(bwd, 'ln_bwd'),
        'c_proj^T GEMM': pick(bwd, 'proj^T'),
        'QuickGELU derivative': pick(bwd, 'quickgelu_bwd'),
        'c_fc^T GEMM': pick(bwd, 'fc^T'),
        'out_proj^T GEMM': pick(bwd, 'out^T'),
        'attention backward (2 launches)': pick(bwd, 'attention_bwd'),
        'q/k/v^T GEMM (K = 3 Wd)': pick(bwd, 'qkv^T'),
        'tokens + ln_pre adjoint': pick(bwd, 'tokens_bwd'),
        'patch embedding^T GEMM': pick(bwd, 'patch^T'),
        'input adjoint (bicubic + affine)': lambda: L.check(L.lib.rick_clip_input_bwd_f32(
            ws.gx0.data_ptr(), gx.data_ptr(), n, 256, 256, c.size, c.patch, L.stream_ptr()), 'rick_clip_input_bwd_f32'),
    }


def torch_reference(p, cfg, x):
    """rick_amd.clip.torch_forward with the patch embedding as a reshape and a matrix product: the same fp32 sums of products
    without a convolution, whose backward pass would first send the library on a search for a 32 x 32 stride-32 kernel."""
    from rick_amd.clip import resize_affine, torch_tower
    n, g, k = x.shape[0], cfg.grid, cfg.patch
    rows = resize_affine(x, cfg.size).reshape(n, 3, g, k, g, k).permute(0, 2, 4, 1, 3, 5).reshape(n, g * g, 3 * k * k)
    return torch_tower(p, cfg, rows @ p['conv1'].reshape(cfg.width, -1).t())


def main_backward(args):
    from rick_amd.clip import ClipImageFeatures, params_from_state_dict
    from tests.clip_f64 import synthetic_clip_state_dict
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev, size = 'cuda', 256
    params = params_from_state_dict(synthetic_clip_state_dict(VIT_B32, 0))
    pd = {k: v.to(dev) for k, v in params.items()}
    res = {'metric': 'clip_vit_b32_backward'}
    for n in args.n:
        t0 = time.time()
        net = ClipImageFeatures(params, device=dev, batch=n).prepare_grad(grad_batch=n)
        cfg = net.cfg
        gen = torch.Generator(dev).manual_seed(n)
        x = (torch.rand(n, 3, size, size, device=dev, generator=gen) * 2 - 1).requires_grad_()
        r = torch.randn(n, cfg.dim, device=dev, generator=gen)
        hip = lambda: torch.autograd.grad((net.encode(x) * r).sum(), x)[0]                    # noqa: E731
        ref = lambda: torch.autograd.grad((torch_reference(pd, cfg, x) * r).sum(), x)[0]      # noqa: E731
        fwd = lambda: net(x.detach())                                                          # noqa: E731
        gh, gt = hip(), ref()
        diff = float((gh - gt).abs().max() / gt.abs().max())
        print(f'n={n}: set up, first pass of both in {time.time() - t0:.1f} s', flush=True)
        timed(hip, 3), timed(ref, 3)                                          # warm-up of both
        th, tt = [], []
        for _ in range(args.rounds):
            th.append(timed(hip, args.iters))
            tt.append(timed(ref, args.iters))
        h, t, f = sorted(th)[len(th) // 2], sorted(tt)[len(tt) // 2], timed(fwd, args.iters)
        res.update({f'hip_fwd_bwd_ms_n{n}': h * 1e3, f'torch_fwd_bwd_ms_n{n}': t * 1e3, f'hip_fwd_only_ms_n{n}': f * 1e3,
                    f'max_rel_grad_diff_vs_torch_n{n}': diff})
        print(f'ViT-B/32 n={n:3d} from {size}^2, forward + backward: HIP kernels {h * 1e3:.2f} ms ({n / h:7.1f} img/s)   torch fp32 autograd '
              f'{t * 1e3:.2f} ms ({n / t:7.1f} img/s)   hip / torch = {h / t:.3f}   forward only (__call__) {f * 1e3:.2f} ms   '
              f'max rel gradient diff {diff:.2e}')
        print('    rounds (ms)  hip: ' + ' '.join(f'{v * 1e3:.2f}' for v in th) + '   torch: ' + ' '.join(f'{v * 1e3:.2f}' for v in tt))
        hip()                                                                 # valid activations and gradients in the workspace
        total = 0.0
        for name, fn in backward_families(net, n).items():
            tf = timed(fn, args.iters)
            total += tf
            res[f'bwd_family_ms_n{n}:{name}'] = tf * 1e3
            print(f'    {name:44s} {tf * 1e3:8.3f} ms')
        print(f'    {"sum of the backward families":44s} {total * 1e3:8.3f} ms', flush=True)
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))


def main_text(args):
    """160 prompts of 77 tokens through ClipTextFeatures at the ViT-B/32 text dimensions, against torch_text_forward on the
    same CUDA tensors."""
    from rick_amd.cliptext import ClipTextFeatures, params_from_state_dict, torch_text_forward
    from tests.cliptext_f64 import synthetic_text_state_dict, text_prompts
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev, n = 'cuda', 160
    params = params_from_state_dict(synthetic_text_state_dict(VIT_B32_TEXT, 0))
    pd = {k: v.to(dev) for k, v in params.items()}
    net = ClipTextFeatures(params, device=dev, batch=n, heads=8)
    cfg = net.cfg
    ids = text_prompts(n, cfg.tokens, cfg.vocab, seed=n).to(dev)
    hip = lambda: net(ids)                                                    # noqa: E731  (validates on the host and uploads, as a user's call does)
    with torch.no_grad():
        ref = lambda: torch_text_forward(pd, cfg, ids)                        # noqa: E731
        diff = float((hip() - ref()).abs().max() / ref().abs().max())
        timed(hip, 3), timed(ref, 3)                                          # warm-up of both
        th, tt = [], []
        for _ in range(args.rounds):
            th.append(timed(hip, args.iters))
            tt.append(timed(ref, args.iters))
    h, t = sorted(th)[len(th) // 2], sorted(tt)[len(tt) // 2]
    res = {'metric': 'clip_vit_b32_text', 'hip_prompts_s': n / h, 'torch_prompts_s': n / t, 'hip_ms': h * 1e3, 'torch_ms': t * 1e3,
           'max_rel_diff_vs_torch': diff}
    print(f'ViT-B/32 text tower, {n} prompts of {cfg.tokens} tokens: HIP kernels {n / h:8.1f} prompts/s ({h * 1e3:.2f} ms)   torch fp32 '
          f'composition {n / t:8.1f} prompts/s ({t * 1e3:.2f} ms)   hip / torch = {h / t:.3f}   max rel diff {diff:.2e}')
    print('    rounds (ms)  hip: ' + ' '.join(f'{v * 1e3:.2f}' for v in th) + '   torch: ' + ' '.join(f'{v * 1e3:.2f}' for v in tt))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20, help='passes per timed round')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--backward', action='store_true', help='time forward + backward of encode instead')
    ap.add_argument('--text', action='store_true', help='time the text tower (rick_amd/cliptext.py) instead')
    ap.add_argument('--n', type=int, nargs='+', default=[4, 8, 25], help='batch sizes of --backward')
    args = ap.parse_args()
    if args.backward:
        return main_backward(args)
    if args.text:
        return main_text(args)
    from rick_amd.clip import ClipImageFeatures, params_from_state_dict, torch_forward
    from tests.clip_f64 import synthetic_clip_state_dict
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    dev, size = 'cuda', 256
    sd = synthetic_clip_state_dict(VIT_B32, 0)
    params = params_from_state_dict(sd)
    pd = {k: v.to(dev) for k, v in params.items()}
    res = {'metric': 'clip_vit_b32'}
    for n in (25, 100):
        net = ClipImageFeatures(params, device=dev, batch=n)
        cfg = net.cfg
        x = torch.rand(n, 3, size, size, device=dev, generator=torch.Generator(dev).manual_seed(n)) * 2 - 1
        hip = lambda: net(x)                                                  # noqa: E731
        with torch.no_grad():
            ref = lambda: torch_forward(pd, cfg, x)                           # noqa: E731
            diff = float((hip() - ref()).abs().max() / ref().abs().max())
            timed(hip, 3), timed(ref, 3)                                      # warm-up of both
            th, tt = [], []
            for _ in range(args.rounds):
                th.append(timed(hip, args.iters))
                tt.append(timed(ref, args.iters))
        h, t = sorted(th)[len(th) // 2], sorted(tt)[len(tt) // 2]
        res.update({f'hip_img_s_n{n}': n / h, f'torch_img_s_n{n}': n / t, f'hip_ms_n{n}': h * 1e3, f'torch_ms_n{n}': t * 1e3,
                    f'max_rel_diff_vs_torch_n{n}': diff})
        print(f'ViT-B/32 n={n:3d} from {size}^2: HIP kernels {n / h:8.1f} img/s ({h * 1e3:.2f} ms)   torch fp32 composition '
              f'{n / t:8.1f} img/s ({t * 1e3:.2f} ms)   hip / torch = {h / t:.3f}   max rel diff {diff:.2e}')
        print('    rounds (ms)  hip: ' + ' '.join(f'{v * 1e3:.2f}' for v in th) + '   torch: ' + ' '.join(f'{v * 1e3:.2f}' for v in tt))
        total = 0.0
        for name, fn in families(net, n, x).items():
            tf = timed(fn, args.iters)
            total += tf
            res[f'family_ms_n{n}:{name}'] = tf * 1e3
            print(f'    {name:36s} {tf * 1e3:8.3f} ms')
        print(f'    {"sum of the families":36s} {total * 1e3:8.3f} ms', flush=True)
        del net
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == '__main__':
    main()
