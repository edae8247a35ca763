"""Singular-value adaptation (rick_amd/svd.py, rick_amd/csrc/svd.hip) on the GPU: apply_ and grads_ over the real generator and
discriminator tables at 256 px next to the same definition composed per layer in torch (permuted copies + torch.bmm), the
achieved TFLOP/s against the f32-MFMA peak, the one-off construction time of the host decompositions, an eager 256-px / batch-4
g_step / d_step with the adapter off and on, and — with --parent DIR — bench.py on the parent commit and on this one in turns.

  python tools/bench_svd.py [--iters 20] [--rounds 5] [--skip-step] [--parent DIR [--headline-rounds 3]]

Each figure is timed by device events around back-to-back CALLS (Python wrapper and launches included) after a warm-up call, over
rotating copies of the gradient / weight buffers, the variants taking turns inside each of `rounds` windows; median and range over
the windows are printed.  FLOP = 2 co ci taps r per layer and direction (the GEMM alone; the torch composition does the same
products).  DIR is a checkout of the parent commit with its library built; both trees run `bench.py --gpus 1 --steps 20
--warmup 5` as fresh child processes.  Prints a readable report and one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_ewc import alternated      # noqa: E402

PEAK_TF = 157.3      # f32 MFMA (= f32 vector) peak of the MI355X


def networks(size=256):
    from rick_amd.models import Discriminator, Generator
    from rick_amd.train import FlatParams, d_optim_filter, g_optim_filter
    g = Generator(size, 512, 8, channel_multiplier=2).cuda()
    d = Discriminator(size).cuda()
    return {'G': FlatParams(g.named_parameters(), g_optim_filter), 'D': FlatParams(d.named_parameters(), d_optim_filter)}


def torch_apply(svd, w):
    """W^ = W0 + U diag(d) Vt per layer: torch.bmm and a permuted copy into the tap-innermost weight."""
    with torch.no_grad():
        for n in svd.names:
            a, b = svd.segment(n)
            delta = torch.bmm(svd.u[n] * svd.d[n][:, None, :], svd.vt[n]).permute(1, 2, 0)
            w[a:b].view(svd.shape3[n]).copy_(svd.snapshot(n) + delta)


def torch_grads(svd, grad):
    """dd = sum_i (U^T G_t) Vt per layer: a permuted copy of G, torch.bmm, an elementwise product and a row sum."""
    with torch.no_grad():
        for n in svd.names:
            a, b = svd.segment(n)
            g = grad[a:b].view(svd.shape3[n]).permute(2, 0, 1).contiguous()
            svd.d[n].grad.copy_((torch.bmm(svd.u[n].transpose(1, 2), g) * svd.vt[n]).sum(2))


def pass_report(args):
    from rick_amd.svd import SvdAdapter, apply_tables, grad_tables
    res = {}
    gen = torch.Generator('cuda').manual_seed(0)
    print(f'us per CALL, median of {args.rounds} alternated windows [min-max]; TFLOP/s = 2 co ci taps r per layer over the median, '
          f'against the {PEAK_TF} TFLOP/s f32-MFMA peak; x = composed-torch time over HIP time')
    for key, flat in networks().items():
        t0 = time.perf_counter()
        svd = SvdAdapter(flat)
        torch.cuda.synchronize()
        res[f'{key}_construct_s'] = time.perf_counter() - t0
        t = svd.tables
        print(f'  {key}: {len(svd.names)} layers, {t.elements / 1e6:.2f} M elements, {t.flops / 1e9:.2f} GFLOP per direction, '
              f'{t.n_apply} / {t.n_grad} blocks; construction (host fp64 decompositions, upload) {res[f"{key}_construct_s"]:.1f} s')
        with torch.no_grad():
            for n in svd.names:
                svd.d[n].copy_(0.1 * svd.s0[n] * torch.randn(svd.d[n].shape, device='cuda', generator=gen))
        n = svd.hi - svd.lo
        grads = [torch.randn(n, device='cuda', generator=gen) for _ in range(2)]
        ws = [torch.empty(n, device='cuda') for _ in range(2)]
        t = alternated({
            'apply': [(lambda w=w: apply_tables(svd.w0, w, svd.u_flat, svd.vt_flat, svd.fac.flat, svd.tables)) for w in ws],
            'grad': [(lambda g=g: grad_tables(g, svd.u_flat, svd.vt_flat, svd.fac.grad, svd.partials, svd.tables)) for g in grads],
            'torch_apply': [(lambda w=w: torch_apply(svd, w)) for w in ws],
            'torch_grad': [(lambda g=g: torch_grads(svd, g)) for g in grads]}, args.iters, args.rounds)
        res[f'{key}_gflop'] = svd.tables.flops / 1e9
        for name in ('apply', 'grad'):
            med, lo, hi = t[name]
            ref = t['torch_' + name][0]
            tf = svd.tables.flops / med / 1e12
            res[f'{key}_{name}_us'] = [v * 1e6 for v in t[name]]
            res[f'{key}_torch_{name}_us'] = [v * 1e6 for v in t['torch_' + name]]
            res[f'{key}_{name}_tflops'] = tf
            print(f'  {key} {name:5s} {med * 1e6:9.1f} us [{lo * 1e6:.1f}-{hi * 1e6:.1f}]  {tf:6.1f} TFLOP/s = {tf / PEAK_TF:.2f} of peak   '
                  f'torch {ref * 1e6:9.1f} us [{t["torch_" + name][1] * 1e6:.1f}-{t["torch_" + name][2] * 1e6:.1f}]  x{ref / med:.2f}',
                  flush=True)
        del svd, grads, ws
        torch.cuda.empty_cache()
    return res


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
    trainers = {}
    for name, on in (('off', False), ('on', True)):
        g, d = make()
        trainers[name] = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, svd_adapt=on), g, d, *make())
    real = torch.randn(B, 3, size, size, device='cuda')
    noise = [torch.randn(B, 512, device='cuda')]
    variants = {}
    for name, tr in trainers.items():
        variants[f'g_step_{name}'] = [lambda tr=tr: tr.g_step(noise)]
        variants[f'd_step_{name}'] = [lambda tr=tr: tr.d_step(real, noise)]
    t = alternated(variants, max(8, args.iters), args.rounds)
    res = {}
    for step in ('g_step', 'd_step'):
        off, on = t[f'{step}_off'], t[f'{step}_on']
        res[f'{step}_eager_ms_svd_off'] = [v * 1e3 for v in off]
        res[f'{step}_eager_ms_svd_on'] = [v * 1e3 for v in on]
        print(f'eager {step} at 256 px, batch {B}: adapter off {off[0] * 1e3:.3f} ms [{off[1] * 1e3:.3f}-{off[2] * 1e3:.3f}]   '
              f'on {on[0] * 1e3:.3f} ms [{on[1] * 1e3:.3f}-{on[2] * 1e3:.3f}]   added {(on[0] - off[0]) * 1e3:.3f} ms', flush=True)
    return res


def headline_report(args):
    """bench.py on the parent commit and on this tree, taking turns, fresh child processes."""
    res = {'parent': [], 'this': []}
    for rnd in range(args.headline_rounds):
        for name, cwd in (('parent', os.path.abspath(args.parent)), ('this', ROOT)):
            out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5'], cwd=cwd,
                                 capture_output=True, text=True, timeout=600)
            line = next((l for l in reversed(out.stdout.splitlines()) if l.startswith('{')), None)
            if out.returncode or line is None:
                raise SystemExit(f'bench.py failed in {cwd}:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}')
            rec = json.loads(line)
            res[name].append(rec.get('value'))
            print(f'headline round {rnd + 1} {name:6s}: {rec.get("metric")} = {rec.get("value")} {rec.get("unit", "")}', flush=True)
    return {'headline_parent': res['parent'], 'headline_this': res['this']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-pass', action='store_true')
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--parent', metavar='DIR', help='a checkout of the parent commit with its library built: run bench.py in both trees')
    ap.add_argument('--headline-rounds', type=int, default=3)
    args = ap.parse_args()
    res = {'metric': 'svd_pass', 'size': 256, 'batch': 4}
    if args.parent:                      # first, in child processes: this process has not opened the GPU yet
        res.update(headline_report(args))
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_svd.py needs an MI355X')
    if not args.skip_pass:
        res.update(pass_report(args))
    if not args.skip_step:
        res.update(step_report(args))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
