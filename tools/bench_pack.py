"""Time of the one-launch weight re-pack of a network (rick_conv_pack_weights_multi) after an optimiser step, on the
steady-state table: one D, G, R1 and path-length step run first, so every view the second-order passes ask for is there.
Per network: views requested (by tag path), distinct views (descriptors), paired views, bytes read + written by the
launch, median time of grp.refresh() and the resulting TB/s."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rick_amd import op
from rick_amd.models import Discriminator, Generator
from rick_amd.synth import synth_reals
from rick_amd.train import RickTrainer, TrainConfig
torch.manual_seed(1)
dev = 'cuda'
g, d = Generator(256, 512, 8).to(dev), Discriminator(256).to(dev)
ge, de = Generator(256, 512, 8).to(dev), Discriminator(256).to(dev)
tr = RickTrainer(TrainConfig(batch=4, num_fisher_img=1), g, d, ge, de)
real = synth_reals(4, 256, seed=1).to(dev)
tr.d_step(real, [torch.randn(4, 512, device=dev)])
tr.g_step([torch.randn(4, 512, device=dev)])
tr.r1_step(real)
tr.plr_step([torch.randn(2, 512, device=dev)])
torch.cuda.synchronize()
for name, grp, flat in (('G', tr._pack_groups[0], tr.g_flat), ('D', tr._pack_groups[1], tr.d_flat)):
    h = grp.host[:grp.n]
    partner = h['partner'] if 'partner' in h.dtype.names else h['reserved']
    distinct = len({(int(r['w']), int(r['s_co']), int(r['s_ci']), int(r['s_t']), int(r['Co']), int(r['Ci']), int(r['nslices']),
                     float(r['scale'])) for r in h})
    written = sum(r['buf'].numel() for r in grp.reqs.values())
    read = 0
    for i, (r, p) in enumerate(zip(h, partner)):
        if p == 0 or p - 1 > i:                                  # a pair reads its source once
            read += 4 * int(r['Co']) * int(r['Ci']) * int(r['nslices'])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(20):
        op.bump_weights_epoch(flat.params)
        e0.record(); grp.refresh(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    us = sorted(ts)[len(ts) // 2]
    requested = len(grp.tags) if hasattr(grp, 'tags') else grp.n
    print(f'{name}: {requested} views requested, {grp.n} descriptors, {distinct} distinct, {int((partner != 0).sum())} paired, '
          f'{grp.total_blocks} per-view blocks, {read / 1e6:.1f} MB read + {written / 1e6:.1f} MB written: '
          f'{us:.1f} us = {(read + written) / us / 1e6:.2f} TB/s')
