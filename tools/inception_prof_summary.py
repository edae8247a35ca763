"""Per-kernel summary of a `rocprofv3 --kernel-trace --stats` run of tools/bench_inception.py (rocpd SQLite output), with the
achieved TFLOP/s of every Inception convolution launch.

  rocprofv3 --kernel-trace --stats -d OUT -o inc -- python tools/bench_inception.py --iters 5 --skip-eval
  python tools/inception_prof_summary.py OUT/inc_results.db > profiles/r07_inception_kernel_stats.txt

The convolution launches are matched to layers by order: every extractor call issues the plan's convolutions in the same
sequence (rick_amd/inception.py: _Plan), and the call's N follows from the launch grid.  FLOPs are the table's algorithmic
2 x multiply-adds (padding columns and rows of the GEMM tiles not counted)."""
import collections
import os
import sqlite3
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def plan_convs():
    """[(label, M per image, Co, K)] of the dims=2048 plan's convolution launches, in issue order (built on the CPU)."""
    from rick_amd import inception as inc
    rec = []

    class Geometry(inc._Plan):                  # records the launches, skips the weight packing
        def _conv(self, us, P, src, h, w, ci, dsts):
            k, s, p = us[0][3], us[0][4], us[0][5]
            oh, ow = inc._out_hw(h, w, k, s, p)
            rec.append(('+'.join(u[0] for u in us), oh * ow, sum(u[2] for u in us), k[0] * k[1] * us[0][1]))

    Geometry({}, 3, 1, 'cpu')
    return rec


def main(db):
    c = sqlite3.connect(db)
    rows = c.execute('select name, duration, grid_x, workgroup_x from kernels order by start').fetchall()
    convs = plan_convs()
    by_name = collections.defaultdict(lambda: [0, 0])
    layer = collections.defaultdict(lambda: [0, 0.0, 0.0])          # (label, N) -> launches, ns, flops
    i = 0
    for name, dur, gx, wg in rows:
        short = name.split('(')[0]
        by_name[short][0] += 1
        by_name[short][1] += dur
        if short.startswith('void inc_conv_kernel') or short.startswith('inc_conv_kernel'):
            label, m_img, co, k = convs[i % len(convs)]
            if i % len(convs) == 0:             # the call's first launch (Conv2d_1a_3x3, 149 x 149 positions per image)
                n = round(gx // wg * 128 / m_img)       # (grid_x counts work-items)
            L = layer[(label, n)]
            L[0] += 1
            L[1] += dur
            L[2] += 2.0 * n * m_img * co * k
            i += 1
    total = sum(v[1] for v in by_name.values())
    print(f'kernel dispatches: {len(rows)}, total kernel time {total / 1e6:.2f} ms')
    print(f'{"kernel":<60} {"calls":>7} {"total ms":>10} {"mean us":>10} {"%":>6}')
    for k, (cnt, ns) in sorted(by_name.items(), key=lambda kv: -kv[1][1])[:25]:
        print(f'{k[:60]:<60} {cnt:>7} {ns / 1e6:>10.3f} {ns / cnt / 1e3:>10.1f} {100 * ns / total:>6.1f}')
    print()
    print('Inception convolutions (inc_conv_kernel), per layer and call size N: achieved TFLOP/s (algorithmic FLOPs)')
    print(f'{"layer (fused heads joined by +)":<92} {"N":>4} {"calls":>5} {"mean us":>9} {"TFLOP/s":>8}')
    agg = collections.defaultdict(lambda: [0.0, 0.0])
    for (label, n), (cnt, ns, fl) in layer.items():
        print(f'{label[:92]:<92} {n:>4} {cnt:>5} {ns / cnt / 1e3:>9.1f} {fl / ns / 1e3:>8.1f}')
        agg[n][0] += ns
        agg[n][1] += fl
    for n, (ns, fl) in sorted(agg.items()):
        print(f'all convolutions at N={n}: {ns / 1e6:.2f} ms, {fl / ns / 1e3:.1f} TFLOP/s')


if __name__ == '__main__':
    main(sys.argv[1])
