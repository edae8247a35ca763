"""DCL's contrastive terms (rick_amd/dcl.py) on the GPU: rick_xgram_f32 and rick_xrowmix_f32 at the 13 feature shapes of the
256-px generator and the 14 of the discriminator at batch 4 (4 rows against 4 rows in two allocations); at the largest generator
shape next to rick_gram_f32 at B = 8 on the same bytes and to the ``cat`` + rick_gram_f32 route a one-tensor kernel would need;
then the trainer's G step and D step at 256 px, batch 4, eager, with each term on and off.

  python tools/bench_dcl.py [--iters 200] [--rounds 5] [--skip-step] [--skip-kernels]

Times are device events around back-to-back CALLS (Python wrapper, workspace allocation and launches included), after a warm-up
call, measured as tools/bench_cdc.py measures them: the variants of a shape take turns inside each of `rounds` windows, the
median and the range over the windows are printed, and each call of a rotation takes the next of several copies of the operands,
enough copies to exceed the 256 MiB the chip can keep between two uses of a line (at most 16: the small layers stay
cache-resident and are launch-bound either way).  GB/s counts both operands read once (xgram) and both read plus one written
(xrowmix): the bytes the algorithm needs over the call time, a call-level figure.  Prints a readable report and one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
from bench_cdc import alternated  # noqa: E402


def cell(t):
    return f'{t[0] * 1e6:8.1f} [{t[1] * 1e6:.1f}-{t[2] * 1e6:.1f}]'


def kernels_report(args, name, feats):
    """feats: a list of [8, ...] tensors; rows [:4] play a, a separate copy of rows [4:] plays b."""
    from rick_amd import cdc, dcl
    dev = feats[0].device
    rows_out = []
    print(f'{name}: us per CALL, median of {args.rounds} alternated windows [min-max]; GB/s = a and b read once (xgram) / a and b read '
          f'and y written once (xrowmix) over the median call time')
    print(f'{"layer":>5} {"shape of a, b":>20} {"MB a+b":>7} | {"xgram us":>22} {"GB/s":>6} | {"xrowmix us":>22} {"GB/s":>6}')
    for l, f in enumerate(feats):
        by = f.numel() * 4                                      # a + b
        copies = max(1, min(16, -(-600 * 2 ** 20 // by)))
        pairs = [(f[:4].clone(memory_format=torch.preserve_format), f[4:].clone(memory_format=torch.preserve_format)) for _ in range(copies)]
        assert all(cdc._sample_dense(a) and cdc._sample_dense(b) and dcl._same_layout(a, b) for a, b in pairs)
        rws = [(cdc._rows(a), cdc._rows(b)) for a, b in pairs]
        outs = [torch.empty_like(rws[0][0]) for _ in range(2)]
        M, d = torch.randn(4, 4, device=dev), torch.randn(4, device=dev)
        iters = args.iters if by < 32 * 2 ** 20 else max(20, args.iters // 4)
        with torch.no_grad():
            t = alternated({
                'xgram': ([(lambda a=a, b=b: dcl.xgram(a, b)) for a, b in pairs], 1.0),
                'xrowmix': ([(lambda k=k, a=a, b=b: dcl.xrowmix(M, d, a, b, out=outs[k % 2])) for k, (a, b) in enumerate(rws)], 1.0)},
                iters, args.rounds)
        gb_x, gb_m = by / t['xgram'][0] / 1e9, 1.5 * by / t['xrowmix'][0] / 1e9
        rows_out.append(dict(layer=l, shape=[4] + list(f.shape[1:]), mbytes=by / 1e6, xgram_us=[v * 1e6 for v in t['xgram']],
                             xgram_call_gbs=gb_x, xrowmix_us=[v * 1e6 for v in t['xrowmix']], xrowmix_call_gbs=gb_m))
        print(f'{l:5d} {str((4,) + tuple(f.shape[1:])):>20} {by / 1e6:7.2f} | {cell(t["xgram"]):>22} {gb_x:6.0f} | '
              f'{cell(t["xrowmix"]):>22} {gb_m:6.0f}', flush=True)
        del pairs, rws, outs
        torch.cuda.empty_cache()
    return rows_out


def against_gram(args, f):
    """xgram(4, 4) on two allocations, rick_gram_f32 at B = 8 on the same bytes in one tensor, and cat + rick_gram_f32."""
    from rick_amd import cdc, dcl
    by = f.numel() * 4
    copies = max(1, min(16, -(-600 * 2 ** 20 // by)))
    pairs = [(f[:4].clone(memory_format=torch.preserve_format), f[4:].clone(memory_format=torch.preserve_format)) for _ in range(copies)]
    whole = [f.clone(memory_format=torch.preserve_format) for _ in range(copies)]
    fmt = torch.channels_last if f.dim() == 4 and f.is_contiguous(memory_format=torch.channels_last) else torch.contiguous_format
    iters = max(20, args.iters // 4)
    with torch.no_grad():
        t = alternated({'xgram': ([(lambda a=a, b=b: dcl.xgram(a, b)) for a, b in pairs], 1.0),
                        'gram8': ([(lambda x=x: cdc.gram(x)) for x in whole], 1.0),
                        'cat_gram': ([(lambda a=a, b=b: cdc.gram(torch.cat([a, b]).contiguous(memory_format=fmt))) for a, b in pairs], 1.0)},
                       iters, args.rounds)
    res = {k: dict(us=[v * 1e6 for v in t[k]], call_gbs=by / t[k][0] / 1e9, call_gbs_range=[by / t[k][2] / 1e9, by / t[k][1] / 1e9])
           for k in t}
    print(f'largest generator shape {tuple(f.shape)}, {by / 1e6:.1f} MB in all: GB/s of the {by / 1e6:.1f} MB over the call time')
    for k, label in (('xgram', 'xgram(4, 4), two allocations'), ('gram8', 'rick_gram_f32, B = 8, one tensor'), ('cat_gram', 'cat + rick_gram_f32')):
        r = res[k]
        print(f'  {label:34s} {cell(t[k])} us   {r["call_gbs"]:6.0f} GB/s [{r["call_gbs_range"][0]:.0f}-{r["call_gbs_range"][1]:.0f}]', flush=True)
    return res


def step_report(args, make):
    from rick_amd.train import RickTrainer, TrainConfig
    res = {}
    B = 4
    trainers = {}
    for name, kw in (('off', {}), ('dcl_g', dict(dcl_g_weight=2.0)), ('dcl_d', dict(dcl_d_weight=0.5))):
        g, d = make()
        g_ema, d_ema = make()
        gs, ds = make()
        trainers[name] = RickTrainer(TrainConfig(size=256, batch=B, warmup_iter=0, dcl_batch=4, **kw), g, d, g_ema, d_ema, g_source=gs,
                                     d_source=ds)
    z = [torch.randn(B, 512, device='cuda')]
    real = torch.rand(B, 3, 256, 256, device='cuda') * 2 - 1
    t = alternated({'g_off': ([lambda: trainers['off'].g_step(z)], 1.0), 'g_on': ([lambda: trainers['dcl_g'].g_step(z)], 1.0),
                    'd_off': ([lambda: trainers['off'].d_step(real, z)], 1.0), 'd_on': ([lambda: trainers['dcl_d'].d_step(real, z)], 1.0)},
                   max(10, args.iters // 10), args.rounds)
    for k, label in (('g_off', 'g_step, CL1 off'), ('g_on', 'g_step, CL1 on '), ('d_off', 'd_step, CL2 off'), ('d_on', 'd_step, CL2 on ')):
        res[f'{k}_eager_ms'] = [v * 1e3 for v in t[k]]
        print(f'{label} (256 px, batch {B}, eager): {t[k][0] * 1e3:.3f} ms [{t[k][1] * 1e3:.3f}-{t[k][2] * 1e3:.3f}]', flush=True)
    res['cl1_cost_ms'] = (t['g_on'][0] - t['g_off'][0]) * 1e3
    res['cl2_cost_ms'] = (t['d_on'][0] - t['d_off'][0]) * 1e3
    print(f'per-step cost: CL1 {res["cl1_cost_ms"]:.3f} ms, CL2 {res["cl2_cost_ms"]:.3f} ms')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--skip-step', action='store_true')
    ap.add_argument('--skip-kernels', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tools/bench_dcl.py needs an MI355X')
    torch.backends.cuda.matmul.allow_tf32 = False
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
    res = {'metric': 'dcl_xgram_xrowmix', 'batch': 4, 'size': size}
    if not args.skip_kernels:
        g, d = make()
        with torch.no_grad():
            img, gf = g([torch.randn(8, 512, device='cuda', generator=torch.Generator('cuda').manual_seed(0))], return_feats=True)
            gf = [f.detach() for f in gf]
            res['generator_layers'] = kernels_report(args, 'generator features', gf)
            res['largest_generator_shape'] = against_gram(args, max(gf, key=lambda f: f.numel()))
            del gf
            torch.cuda.empty_cache()
        d.requires_grad_(True)                                  # the D step's pass: with gradients, both calls in one batch
        df = [f.detach() for f in d(img.detach(), calls=2)[1]]
        del g, d, img
        torch.cuda.empty_cache()
        res['discriminator_layers'] = kernels_report(args, 'discriminator features', df)
        del df
        torch.cuda.empty_cache()
    if not args.skip_step:
        res.update(step_report(args, make))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
