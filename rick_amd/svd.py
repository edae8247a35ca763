"""Singular-value adaptation (Robb et al., "Few-Shot Adaptation of Generative Adversarial Networks", 2020: FSGAN) on the flat
parameter buffers.  FSGAN freezes the singular vectors of every pretrained weight matrix and trains only the singular values.  The
paper and its code were not at hand when this was written: this docstring is the specification that is built.

A weight is viewed as W[co, ci, taps] (4-D conv weights as [co, ci, kh kw]; the generator's 5-D [1, co, ci, 3, 3] without the
leading 1; a 2-D weight has taps = 1).  For every tap t the matrix W[:, :, t] is decomposed ONCE, at construction, by
torch.linalg.svd in fp64 on the host (full_matrices=False, r = min(co, ci)); the factors are stored rounded to fp32, U[t, co, r]
and Vt[t, r, ci], next to a snapshot W0 of the weight and the source singular values s0[t, r].  The learnt quantity is the SHIFT
of the singular values, d[t, r], initialised to 0:

    W^[o,i,t] = W0[o,i,t] + sum_k U[t,o,k] d[t,k] Vt[t,k,i]
    dd[t,k]   = sum_o sum_i U[t,o,k] G[o,i,t] Vt[t,k,i]                    G = dL/dW^ as it lies in flat.grad

The delta form is deliberate: W0 + U diag(s0 + d) Vt - U diag(s0) Vt is the same model, but at d = 0 the delta form returns the
source weights exactly and its rounding error scales with |d|, not with |s0|.  singular_values(name) returns s0 + d for
inspection; d is not constrained in sign.  The definition is in terms of the STORED fp32 U and Vt: their departure from
orthogonality (near 1e-7) is part of the model, not an error.

    svd = SvdAdapter(trainer.g_flat)                       # every tensor of the optimised slice with at least two dims
    g_optim.set_mask(svd.frozen_mask())                    # bit 0 on the whole slice: only singular values train
    ... backward, gradient exchange ...
    svd.grads_()                                           # d.grad from flat.grad
    ... the network's masked Adam (the freeze bit leaves the adapted weights alone) ...
    svd.adam_step(); svd.apply_()                          # or svd.step() = grads_, adam_step, apply_

The flat buffer simply holds W^: every convolution form, weight pack, EMA and checkpoint works on it unchanged.  On the device
grads_ and apply_ are the launches of rick_amd/csrc/svd.hip (include/rick_hip.h "SVD"): all layers in one launch each on the
fp32 MFMA, no atomics, bit-identical from run to run and independent of a layer's place in the table.  CPU tensors take the same
definition composed from torch ops in fp64.  Everything an adapter of the slice has in common — names, views, the factors' own
FlatParams and Adam, the step bracket, the state_dict round trip — is rick_amd/adapter.py's FlatAdapter."""
import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib
from .adapter import FlatAdapter, flat_f32, upload_table


class SvdTables:
    """What the launches are driven by (include/rick_hip.h "SVD"), staged on the host and uploaded once: the layer table (the
    host copy is what the entry points validate) and the (layer, tile) list of every block of the apply and of the grad launch.
    specs: one dict per layer with off (first element of the weight in w / w0 / grad), u_off, vt_off, d_off and shape
    (co, ci, taps)."""

    def __init__(self, specs, device):
        if not specs:
            raise ValueError('svd: no layer')
        rec = (_lib.SvdLayer * len(specs))()
        ab, gb, part, flops = [], [], 0, 0
        for k, sp in enumerate(specs):
            co, ci, taps = (int(x) for x in sp['shape'])
            na, ng = _lib.lib.rick_svd_apply_tiles(co, ci, taps), _lib.lib.rick_svd_grad_tiles(co, ci, taps)
            if na < 0 or ng < 0:
                raise ValueError(f'svd: layer {k} has the shape {(co, ci, taps)}; co, ci >= 1 and 1 <= taps <= 16 are supported')
            L = rec[k]
            L.off, L.u_off, L.vt_off, L.d_off, L.part_off = int(sp['off']), int(sp['u_off']), int(sp['vt_off']), int(sp['d_off']), part
            L.co, L.ci, L.taps, L.r = co, ci, taps, min(co, ci)
            part += int(_lib.lib.rick_svd_partials(co, ci, taps))
            ab.extend((k, t) for t in range(na))
            gb.extend((k, t) for t in range(ng))
            flops += 2 * co * ci * taps * min(co, ci)
        self.nlayers, self.layers_host = len(specs), rec
        self.n_apply, self.n_grad, self.npart, self.flops = len(ab), len(gb), part, flops      # flops: of one apply (= one grad)
        self.elements = int(sum(int(np.prod(sp['shape'])) for sp in specs))
        if torch.device(device).type != 'cuda':
            return
        self.layers_dev = upload_table(rec, device)
        self.apply_blocks_dev = torch.tensor(ab, dtype=torch.int32).reshape(-1).to(device)
        self.grad_blocks_dev = torch.tensor(gb, dtype=torch.int32).reshape(-1).to(device)

    def host_ptr(self):
        return ctypes.addressof(self.layers_host)


def apply_tables(w0, w, u, vt, d, tables):
    """rick_svd_apply_f32 on raw buffers: W^ of every layer of the table into `w` (the layout of `w0`)."""
    flat_f32('svd', 'w0, w, u, vt and d', w0, w, u, vt, d)
    if w.numel() != w0.numel():
        raise ValueError('svd: w and w0 must have one length')
    if tables.layers_dev.device != w0.device:
        raise ValueError('svd: the tables live on another device')
    with torch.cuda.device(w0.device):
        _lib.check(_lib.lib.rick_svd_apply_f32(_lib.ptr(w0), _lib.ptr(w), w0.numel(), _lib.ptr(u), u.numel(), _lib.ptr(vt), vt.numel(),
                                               _lib.ptr(d), d.numel(), _lib.ptr(tables.layers_dev), tables.host_ptr(), tables.nlayers,
                                               _lib.ptr(tables.apply_blocks_dev), tables.n_apply, _lib.stream_ptr()),
                   'rick_svd_apply_f32')


def grad_tables(grad, u, vt, dd, partials, tables):
    """rick_svd_grad_f32 + rick_svd_grad_finish_f32 on raw buffers: dd of every layer into `dd` (the layout of d).  partials: fp32
    workspace of at least tables.npart entries."""
    flat_f32('svd', 'grad, u, vt, dd and partials', grad, u, vt, dd, partials)
    if partials.numel() < tables.npart:
        raise ValueError('svd: partials must hold tables.npart entries')
    if tables.layers_dev.device != grad.device:
        raise ValueError('svd: the tables live on another device')
    with torch.cuda.device(grad.device):
        _lib.check(_lib.lib.rick_svd_grad_f32(_lib.ptr(grad), grad.numel(), _lib.ptr(u), u.numel(), _lib.ptr(vt), vt.numel(),
                                              _lib.ptr(partials), partials.numel(), _lib.ptr(tables.layers_dev), tables.host_ptr(),
                                              tables.nlayers, _lib.ptr(tables.grad_blocks_dev), tables.n_grad, _lib.stream_ptr()),
                   'rick_svd_grad_f32')
        _lib.check(_lib.lib.rick_svd_grad_finish_f32(_lib.ptr(partials), partials.numel(), _lib.ptr(dd), dd.numel(),
                                                     _lib.ptr(tables.layers_dev), tables.host_ptr(), tables.nlayers,
                                                     _lib.stream_ptr()), 'rick_svd_grad_finish_f32')


def compose_apply(w0, u, vt, d):
    """W^ [co, ci, taps] in fp64 from torch ops: the definition on W0 [co, ci, taps], U [taps, co, r], Vt [taps, r, ci], d [taps, r]."""
    u, vt, d = u.double(), vt.double(), d.double()
    return w0.double() + torch.bmm(u * d[:, None, :], vt).permute(1, 2, 0)


def compose_grad(g, u, vt):
    """dd [taps, r] in fp64 from torch ops: the definition on G [co, ci, taps], U and Vt."""
    t = torch.bmm(u.double().transpose(1, 2), g.double().permute(2, 0, 1))          # T[t, k, i]
    return (t * vt.double()).sum(2)


def decompose(w3):
    """(U [taps, co, r], s0 [taps, r], Vt [taps, r, ci]) of a [co, ci, taps] weight: torch.linalg.svd in fp64 on the host, per
    tap, rounded to fp32."""
    m = w3.detach().to('cpu', torch.float64).permute(2, 0, 1).contiguous()
    U, S, Vh = torch.linalg.svd(m, full_matrices=False)
    return U.to(torch.float32).contiguous(), S.to(torch.float32).contiguous(), Vh.to(torch.float32).contiguous()


class SvdAdapter(FlatAdapter):
    """The FSGAN adapter over the optimised slice ``[flat.lo:flat.hi]`` of a FlatParams.

    flat: the FlatParams.  names: the adapted parameters (default: every parameter of the slice with ``dim() >= 2``).  lr / betas:
    of the adapter's own Adam.

    Owns W0 (``w0``: fp32, a copy of the slice as it was at construction), the frozen factors (``u[name]`` [taps, co, r],
    ``vt[name]`` [taps, r, ci]: views of the flat buffers ``u_flat`` / ``vt_flat``), the source singular values (``s0[name]``
    [taps, r]), the shifts (``d[name]``: nn.Parameters [taps, r] inside ``fac``, a FlatParams), their optimiser (``optim``) and,
    on the device, the tables and the partials workspace."""

    def __init__(self, flat, names=None, lr=0.002, betas=(0.0, 0.99)):
        super().__init__(flat, names, 'svd', lambda p: p.dim() >= 2)
        names = self.names
        self.rank = {n: min(s[0], s[1]) for n, s in self.shape3.items()}
        self.w0 = flat.flat[self.lo:self.hi].detach().clone()
        us, vts, self.s0, self._uoff, self._vtoff = [], [], {}, {}, {}
        upos = vpos = 0
        for n in names:
            U, S, Vh = decompose(self._w3(self.w0, n))
            self._uoff[n], self._vtoff[n] = upos, vpos
            upos, vpos = upos + U.numel(), vpos + Vh.numel()
            us.append(U.reshape(-1))
            vts.append(Vh.reshape(-1))
            self.s0[n] = S.to(self.device)
        self.u_flat, self.vt_flat = torch.cat(us).to(self.device), torch.cat(vts).to(self.device)
        self.u = {n: self.u_flat[self._uoff[n]:self._uoff[n] + s[2] * s[0] * self.rank[n]].view(s[2], s[0], self.rank[n])
                  for n, s in self.shape3.items()}
        self.vt = {n: self.vt_flat[self._vtoff[n]:self._vtoff[n] + s[2] * self.rank[n] * s[1]].view(s[2], self.rank[n], s[1])
                   for n, s in self.shape3.items()}
        self._own_factors([(f'd.{n}', nn.Parameter(torch.zeros(self.shape3[n][2], self.rank[n], device=self.device)))
                           for n in names], lr, betas)
        self.d = {n: self.fac.params[self.fac.index[f'd.{n}']] for n in names}
        specs = [dict(off=self.segment(n)[0], u_off=self._uoff[n], vt_off=self._vtoff[n], d_off=self.fac_range(f'd.{n}')[0],
                      shape=self.shape3[n]) for n in names]
        self.tables = SvdTables(specs, self.device)
        self.partials = torch.zeros(self.tables.npart, device=self.device, dtype=torch.float32) if self.w0.is_cuda else None

    def singular_values(self, name):
        """s0 + d, [taps, r] (fp32): the singular values of the adapted weight along the frozen directions."""
        return self.s0[name] + self.d[name].detach()

    def frozen_mask(self, rest=False):
        """The uint8 mask for the NETWORK's own MaskedFlatAdam (one byte per element of flat.flat).  Bit 0 (freeze) is set on every
        adapted element — their only way to move is apply_().  rest=False: also on everything else in the optimised slice (FSGAN
        trains only singular values); rest=True leaves the biases and other non-adapted tensors to the network's optimiser."""
        mask = torch.zeros(self.flat.total, dtype=torch.uint8, device=self.device)
        if not rest:
            mask[self.lo:self.hi] = 1
        for n in self.names:
            lo, hi = self.flat.segment(n)
            mask[lo:hi] = 1
        return mask

    # ---- the two passes
    def _grads_dev(self):
        grad_tables(self.flat.grad[self.lo:self.hi], self.u_flat, self.vt_flat, self.fac.grad, self.partials, self.tables)

    def _apply_dev(self):
        apply_tables(self.w0, self.flat.flat[self.lo:self.hi], self.u_flat, self.vt_flat, self.fac.flat, self.tables)

    def _grads_cpu(self):
        with torch.no_grad():
            for n in self.names:
                self.d[n].grad.copy_(compose_grad(self.grad(n), self.u[n], self.vt[n]))

    def _apply_cpu(self):
        with torch.no_grad():
            for n in self.names:
                self.weight(n).copy_(compose_apply(self.snapshot(n), self.u[n], self.vt[n], self.d[n].detach()).to(torch.float32))

    # ---- persistence: 'w0.<name>' (the parameter's shape), 'u.<name>' [taps, co, r], 'vt.<name>' [taps, r, ci], 's0.<name>',
    # 'd.<name>' and the Adam moments 'm.d.<name>', 'v.d.<name>' [taps, r], and 'steps' (one count per d)
    def _entries(self):
        out = []
        for n in self.names:
            a, b = self.segment(n)
            lo, hi, shape = self.fac_range(f'd.{n}')
            tensors = [(f'w0.{n}', tuple(self.flat.params[self.flat.index[n]].shape), self.w0[a:b]),
                       (f'u.{n}', tuple(self.u[n].shape), self.u[n]), (f'vt.{n}', tuple(self.vt[n].shape), self.vt[n]),
                       (f's0.{n}', shape, self.s0[n]), (f'd.{n}', shape, self.fac.flat[lo:hi]),
                       (f'm.d.{n}', shape, self.optim.m[lo:hi]), (f'v.d.{n}', shape, self.optim.v[lo:hi])]
            out += [(key, sh, torch.float32, dst) for key, sh, dst in tensors]
        return out


