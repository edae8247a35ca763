"""The flat parameter buffers: a network's parameters and gradients re-homed in one fp32 buffer each (FlatParams), the masked Adam
and the EMA that run over them in one launch, and the on-device grad^2 accumulator of the Fisher sweep."""
import numpy as np
import torch

from . import op
from ._lib import check, lib, ptr, stream_ptr

FLAT_ALIGN = 64      # floats


class FlatParams:
    """Re-homes the parameters of a network into ONE flat fp32 buffer (each parameter becomes a view)
    with a matching flat gradient buffer (``p.grad`` are views too).  `opt_filter` marks the parameters an
    optimiser owns; they must be contiguous in registration order (true for both reference networks:
    ``convs.*`` of G, ``convs.1-6 + final_*`` of D) so that one kernel covers mask + Adam of the whole
    slice, one memset zeroes its gradients, RCCL reduces contiguous buckets, and one kernel does the EMA
    of the entire network."""

    def __init__(self, named_params, opt_filter=None):
        named_params = list(named_params)
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        sizes = [p.numel() for p in self.params]
        # every parameter starts on a 256-byte boundary (a bias that follows the 1-element noise strength would
        # otherwise be misaligned for the float4 kernels); offsets[i + 1] is the START of parameter i + 1, the
        # padding in between stays zero (zero gradient: Adam, EMA and the all-reduce leave it zero)
        self.sizes = sizes
        starts, pos = [], 0
        for n in sizes:
            starts.append(pos)
            pos += (n + FLAT_ALIGN - 1) // FLAT_ALIGN * FLAT_ALIGN
        self.offsets = np.array(starts + [pos], dtype=np.int64)
        self.total = int(self.offsets[-1])
        dev = self.params[0].device
        self.flat = torch.zeros(self.total, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(self.total, device=dev, dtype=torch.float32)
        for p, o, n in zip(self.params, self.offsets, sizes):
            self.flat[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + n].view(p.shape)
            p.grad = self.grad[o:o + n].view(p.shape)
        self.index = {n: i for i, n in enumerate(self.names)}
        self.opt_idx = [i for i, n in enumerate(self.names) if opt_filter is None or opt_filter(n)]
        if self.opt_idx and self.opt_idx != list(range(self.opt_idx[0], self.opt_idx[-1] + 1)):
            raise RuntimeError('FlatParams: optimised parameters must be contiguous in registration order')
        self.lo = int(self.offsets[self.opt_idx[0]]) if self.opt_idx else 0
        self.hi = int(self.offsets[self.opt_idx[-1] + 1]) if self.opt_idx else 0

    def zero_grad(self):
        self.grad[self.lo:self.hi].zero_()

    def segment(self, name):
        i = self.index[name]
        return int(self.offsets[i]), int(self.offsets[i]) + self.sizes[i]


class MaskedFlatAdam:
    """torch.optim.Adam(lr, betas, eps=1e-8) over the optimised slice of a FlatParams, with RICK's
    freeze / prune masks applied in the same kernel (train_dynamic_update_prune.py:427-438, 522-540).
    Parameters whose ``requires_grad`` is False at step time are skipped exactly like torch skips
    ``grad is None`` (per-parameter step counts, used by the warm-up stage :202-211)."""

    def __init__(self, flat, lr, betas, eps=1e-8):
        self.fp, self.lr, self.betas, self.eps = flat, lr, betas, eps
        self.m = torch.zeros_like(flat.flat)
        self.v = torch.zeros_like(flat.flat)
        self.steps = [0] * len(flat.params)          # host mirror of steps_dev (checkpoints, run grouping)
        # step counters and bias corrections also live on the device (rick_adam_prepare_f32), so an optimiser step
        # depends on device state only and a captured hipGraph of a whole train step can be replayed
        self.steps_dev = torch.zeros(len(flat.params), device=flat.flat.device, dtype=torch.int32)
        self.bc = torch.ones(8, 2, device=flat.flat.device, dtype=torch.float32)      # one row per run of equal step count
        self.mask = None            # uint8 flat: bit0 freeze, bit1 prune
        self.before_step = None     # callable run at the top of step(): a term added to flat.grad after the gradient exchange
        self.last_runs = []         # [(first param, last param)] of the most recent step()

    def set_mask(self, mask):
        if self.mask is not None and self.mask.shape == mask.shape:
            self.mask.copy_(mask)   # in place: launches captured in a graph keep reading the same buffer
        else:
            self.mask = mask

    def sync_steps_to_device(self):
        self.steps_dev.copy_(torch.tensor(self.steps, dtype=torch.int32))

    def note_replayed_step(self):
        """A captured step() was replayed: the device counters advanced, mirror it on the host."""
        for i0, i1 in self.last_runs:
            for i in range(i0, i1 + 1):
                self.steps[i] += 1

    def step(self):
        if self.before_step is not None:
            self.before_step()
        fp = self.fp
        idx = fp.opt_idx
        active = {i: fp.params[i].requires_grad for i in idx}
        k, n = 0, len(idx)
        runs = []
        while k < n:
            i = idx[k]
            if not active[i]:
                k += 1
                continue
            kk = k
            self.steps[i] += 1
            while kk + 1 < n and active[idx[kk + 1]] and self.steps[idx[kk + 1]] + 1 == self.steps[i]:
                kk += 1
                self.steps[idx[kk]] += 1
            lo, hi = int(fp.offsets[i]), int(fp.offsets[idx[kk] + 1])
            b1, b2 = self.betas
            mk = None if self.mask is None else self.mask[lo:hi]
            if len(runs) >= self.bc.shape[0]:
                raise RuntimeError('MaskedFlatAdam: too many runs of distinct step counts')
            bc = self.bc[len(runs)]
            check(lib.rick_adam_prepare_f32(ptr(self.steps_dev), i, idx[kk] - i + 1, b1, b2, ptr(bc), stream_ptr()),
                  'rick_adam_prepare_f32')
            from .op.conv import hbm_launch
            check(hbm_launch('masked_adam', (28 + (1 if mk is not None else 0)) * (hi - lo), lib.rick_masked_adam_dev_f32,
                             ptr(fp.flat[lo:hi]), ptr(fp.grad[lo:hi]), ptr(self.m[lo:hi]), ptr(self.v[lo:hi]), ptr(mk), hi - lo,
                             self.lr, b1, b2, self.eps, ptr(bc), stream_ptr()), 'rick_masked_adam_dev_f32')
            runs.append((i, idx[kk]))
            k = kk + 1
        self.last_runs = runs
        op.bump_weights_epoch(fp.params)


def ema_flat(ema_flat_params, flat_params, decay):
    """accumulate() of the reference (train_dynamic_update_prune.py:68-73) over every parameter of a
    network in ONE launch (both sides are FlatParams with the same layout)."""
    if ema_flat_params.total != flat_params.total:
        raise RuntimeError('ema_flat: layouts differ')
    check(lib.rick_ema_f32(ptr(ema_flat_params.flat), ptr(flat_params.flat), flat_params.total, decay, stream_ptr()),
          'rick_ema_f32')
    op.bump_weights_epoch(ema_flat_params.params)


class FisherAccumulator:
    """Device-side replacement for the per-sample ``.cpu().numpy()`` accumulation of grad^2
    (train_dynamic_update_prune.py:252-263): acc += g^2 in one fused kernel per tensor."""

    def __init__(self, named_params):
        self.names = [n for n, _ in named_params]
        self.acc = {n: torch.zeros_like(p, memory_format=torch.contiguous_format) for n, p in named_params}

    def add(self, grads):
        for n, g in zip(self.names, grads):
            if g is None:
                continue
            g = g.contiguous()
            check(lib.rick_sq_accumulate_f32(ptr(self.acc[n]), ptr(g), g.numel(), stream_ptr()),
                  'rick_sq_accumulate_f32')

    def scale_(self, s):
        for v in self.acc.values():
            v.mul_(s)

    def zero_(self):
        for v in self.acc.values():
            v.zero_()
