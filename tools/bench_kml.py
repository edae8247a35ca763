"""Kernel modulation (rick_amd/kml.py, rick_amd/csrc/kml.hip) on the GPU: apply_ and grads_ over the real generator and
discriminator slices at 256 px with 0 %, 40 % and 100 % of the rows flagged, next to the same definition composed per layer from
torch broadcasting and autograd; and an eager 256-px / batch-4 iteration with kml_rank = 2 against kml_rank = 0.

  python tools/bench_kml.py [--iters 100] [--rounds 5] [--rank 2] [--skip-step]

Each figure is timed by device events around back-to-back CALLS (Python wrapper and launches included) after a warm-up call, the
variants taking turns inside each of `rounds` windows; median and range over the windows are printed.  GB/s counts the bytes the
algorithm needs — 8 B per modulated element, in either direction — over the call time: a call-level figure, set against the masked
Adam's in-situ 0.72 of the 8 TB/s peak as a yardstick.  A variant's calls run back to back on the same buffers: at 40 % the
streams of one network (about 80 MB) stay in the 256 MiB cache between calls, at 100 % of the generator (190 MB) they mostly do
not — read the GB/s with that in mind.  Prints a readable report and one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_ewc import alternated      # noqa: E402

PEAK_GBS = 8000.0


def networks(size=256):
    from rick_amd.models import Discriminator, Generator
    from rick_amd.train import FlatParams, d_optim_filter, g_optim_filter
    g = Generator(size, 512, 8, channel_multiplier=2).cuda()
    d = Discriminator(size).cuda()
    return {'G': FlatParams(g.named_parameters(), g_optim_filter), 'D': FlatParams(d.named_parameters(), d_optim_filter)}


def flag(kml, fraction, seed=0):
    rng = np.random.RandomState(seed)
    rows = {}
    for n in kml.names:
        co = kml.shape3[n][0]
        f = np.zeros(co, dtype=bool)
        f[rng.permutation(co)[:int(round(fraction * co))]] = True
        rows[n] = torch.from_numpy(f)
    kml.set_rows(rows)


def torch_apply(kml):
    """W^ = W0 (1 + a b^T) on the flagged rows, per layer, from torch broadcasting."""
    with torch.no_grad():
        for n in kml.names:
            idx = kml._bench_idx[n]
            if idx.numel():
                m = 1.0 + kml.a[n][idx] @ kml.b[n].t()
                kml.weight(n)[idx] = kml.snapshot(n)[idx] * m[:, :, None]


def torch_grads(kml):
    """da, db per layer through autograd of sum(G W0 (1 + a b^T)) over the flagged rows."""
    for n in kml.names:
        idx = kml._bench_idx[n]
        a, b = kml.a[n], kml.b[n]
        if not idx.numel():
            a.grad.zero_()
            b.grad.zero_()
            continue
        w = kml.snapshot(n)[idx] * (1.0 + a[idx] @ b.t())[:, :, None]
        ga, gb = torch.autograd.grad((w * kml.grad(n)[idx]).sum(), (a, b))
        a.grad.copy_(ga)
        b.grad.copy_(gb)


def pass_report(args):
    from rick_amd.kml import KmlState
    flats = networks()
    res = {}
    states = {k: KmlState(f, args.rank) for k, f in flats.items()}
    gen = torch.Generator('cuda').manual_seed(0)
    for k, f in flats.items():
        f.grad.copy_(torch.randn(f.grad.shape, device='cuda', generator=gen))
    print(f'rank {args.rank}; us per CALL, median of {args.rounds} alternated windows [min-max]; GB/s = 8 B per modulated element '
          f'over the median; x = composed-torch time over HIP time')
    for frac in (0.0, 0.4, 1.0):
        for key, kml in states.items():
            flag(kml, frac)
            with torch.no_grad():
                for n in kml.names:
                    kml.a[n].copy_(0.1 * torch.randn(kml.a[n].shape, device='cuda', generator=gen) * kml.rows[n][:, None])
            kml._bench_idx = {n: torch.nonzero(kml.rows[n]).view(-1) for n in kml.names}
            t = alternated({'apply': [kml.apply_], 'grad': [kml.grads_], 'torch_apply': [lambda kml=kml: torch_apply(kml)],
                            'torch_grad': [lambda kml=kml: torch_grads(kml)]}, args.iters, args.rounds)
            nbytes = 8 * kml.elements
            tag = f'{key}_{int(frac * 100)}'
            res[f'{tag}_elements'] = kml.elements
            res[f'{tag}_rows'] = kml.flagged
            for name in ('apply', 'grad'):
                med, lo, hi = t[name]
                ref = t['torch_' + name][0]
                gbs = nbytes / med / 1e9
                res[f'{tag}_{name}_us'] = [v * 1e6 for v in t[name]]
                res[f'{tag}_torch_{name}_us'] = [v * 1e6 for v in t['torch_' + name]]
                res[f'{tag}_{name}_gbs'] = gbs
                print(f'  {key} {int(frac * 100):3d} % ({kml.flagged:5d} rows, {kml.elements / 1e6:6.2f} M elements, {kml.nblocks:5d} blocks) '
                      f'{name:5s} {med * 1e6:8.1f} us [{lo * 1e6:.1f}-{hi * 1e6:.1f}]  {gbs:6.0f} GB/s = {gbs / PEAK_GBS:.2f} of peak   '
                      f'torch {ref * 1e6:8.1f} us  x{ref / med:.1f}', flush=True)
    return res


def step_report(args):
    from rick_amd.models import Discriminator, Generator
    from rick_amd.synth import synth_state_dict
    from rick_amd.train import RickTrainer, TrainConfig, build_mask
    from tests.shapes import discriminator_shapes, generator_shapes
    size, B = 256, 4
    sg, sd = synth_state_dict(generator_shapes(size)), synth_state_dict(discriminator_shapes(size))

    def make():
        g, d = Generator(size, 512, 8, channel_multiplier=2), Discriminator(size)
        g.load_state_dict(sg, strict=False)
        d.load_state_dict(sd, strict=False)
        return g.cuda(), d.cuda()
    trainers = {}
    for name, rank in (('off', 0), ('on', args.rank)):
        g, d = make()
        tr = RickTrainer(TrainConfig(size=size, batch=B, warmup_iter=0, kml_rank=rank), g, d, *make())
        # the decision of a sweep at the default quantile: 60 % of the filters of every conv weight frozen
        rng = np.random.RandomState(0)
        for flat, opt, which in ((tr.g_flat, tr.g_optim, 'g'), (tr.d_flat, tr.d_optim, 'd')):
            freeze = {}
            for i in flat.opt_idx:
                p = flat.params[i]
                if p.dim() >= 4 and 'final' not in flat.names[i]:
                    co = p.shape[1] if p.dim() == 5 else p.shape[0]
                    freeze[flat.names[i]] = np.sort(rng.permutation(co)[:int(0.6 * co)])
            zero = {k: v[:0] for k, v in freeze.items()}
            setattr(tr, f'idx_freeze_{which}', freeze)
            setattr(tr, f'zero_idx_{which}', zero)
            opt.set_mask(build_mask(flat, freeze, zero))
        tr.kml_rows_from_masks()
        trainers[name] = tr
    real = torch.randn(B, 3, size, size, device='cuda')
    counter = {k: 0 for k in trainers}

    def it(name):
        counter[name] += 1
        trainers[name].iteration(10 ** 6 + counter[name], real)      # every 4th / 16th iteration carries the regularisers
    t = alternated({k: [(lambda k=k: it(k))] for k in trainers}, max(16, args.iters // 4), args.rounds)
    res = {}
    for name in ('off', 'on'):
        res[f'iteration_eager_ms_kml_{name}'] = [v * 1e3 for v in t[name]]
        print(f'eager iteration at 256 px, batch {B}, kml {name}: {t[name][0] * 1e3:.3f} ms [{t[name][1] * 1e3:.3f}-{t[name][2] * 1e3:.3f}]',
              flush=True)
    res['iteration_eager_ms_added'] = (t['on'][0] - t['off'][0]) * 1e3
    res['kml_rows'] = [trainers['on'].kml_g.flagged, trainers['on'].kml_d.flagged]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--rank', type=int, default=2)
    ap.add_argument('--skip-step', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_kml.py needs an MI355X')
    res = {'metric': 'kml_pass', 'size': 256, 'batch': 4, 'rank': args.rank}
    res.update(pass_report(args))
    torch.cuda.empty_cache()
    if not args.skip_step:
        res.update(step_report(args))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
