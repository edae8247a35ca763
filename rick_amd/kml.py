"""Kernel modulation of the frozen filters (Zhao et al., "Few-shot Image Generation via Adaptation-Aware Kernel Modulation",
NeurIPS 2022: AdAM's rank-constrained KML) on the flat parameter buffers.  RICK freezes the filters whose Fisher information is
high; KML keeps such a filter's source weights W0 and learns a low-rank multiplicative modulation of them.  A weight is viewed as
W[co, ci, taps] (4-D conv weights as [co, ci, kh kw]; the generator's 5-D [1, co, ci, 3, 3] without the leading 1); every layer
has factors a[co, R], b[ci, R], a per-filter flag rows[co] and a snapshot W0:

    s[o,i]    = sum_r a[o,r] b[i,r]
    W^[o,i,t] = W0[o,i,t] (1 + s[o,i])                    rows[o] = 1 (other rows: the live weight, untouched)
    P[o,i]    = sum_t G[o,i,t] W0[o,i,t]                  G = dL/dW^ as it lies in flat.grad
    da[o,r]   = sum_i P[o,i] b[i,r]                       (0 for rows[o] = 0)
    db[i,r]   = sum_{o: rows[o] = 1} P[o,i] a[o,r]

a starts at 0, b ~ N(0, 1): the first W^ is W0 bit for bit and da is non-zero from the first step.

    kml = KmlState(trainer.g_flat, rank=2)                 # convs.*.conv.weight of G; the 3x3 convolutions and 1x1 skips of D
    kml.set_rows({name: bool[co]})                         # entering rows: W0 := the live row, a := 0, Adam moments of a := 0
    ... backward, gradient exchange ...
    kml.grads_()                                           # a.grad, b.grad from flat.grad and W0
    ... the network's masked Adam (the freeze bit leaves the flagged rows alone) ...
    kml.adam_step(); kml.apply_()                          # or kml.step() = grads_, adam_step, apply_

The flat buffer simply holds the modulated weights: every convolution form, weight pack and gradient kernel works on them
unchanged.  On the device grads_ and apply_ are the launches of rick_amd/csrc/kml.hip (include/rick_hip.h "KML"): all layers in one
launch each, 8 B per modulated element, work proportional to the flagged rows, no atomics, bit-identical from run to run.  CPU
tensors take the same definition composed from torch ops in fp64.  a and b are nn.Parameters re-homed in a FlatParams of their own
and stepped by a MaskedFlatAdam (the network's lr and betas by default)."""
import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib

MAX_RANK = 8


class _NoPack:
    """Stands in for a PackGroup on the factors: MaskedFlatAdam.step reports the parameters it updated to op.bump_weights_epoch,
    which invalidates EVERY packed weight when one of them belongs to no group — the factors are never packed."""
    epoch = 0


def _view3(p):
    """(co, ci, taps) of a weight tensor."""
    shape = tuple(p.shape)
    if len(shape) == 5:
        if shape[0] != 1:
            raise ValueError(f'kml: a 5-D weight needs a leading dim of 1, got {shape}')
        shape = shape[1:]
    if len(shape) < 2:
        raise ValueError(f'kml: a weight needs at least two dims, got {shape}')
    return shape[0], shape[1], int(np.prod(shape[2:], dtype=np.int64))


class KmlTables:
    """What the launches are driven by (include/rick_hip.h "KML"), staged on the host and uploaded once: the layer table, the
    compacted lists of flagged rows, the (layer, group) pair of every block and the row flags.  specs: one dict per layer with
    off (first element of the weight in w / w0 / grad), a_off, b_off (first element of a / b in the factor buffer), shape
    (co, ci, taps) and rows (bool [co], NumPy)."""

    def __init__(self, specs, rank, device):
        rec = (_lib.KmlLayer * len(specs))()
        rows, blocks, flags = [], [], []
        part = 0
        for k, sp in enumerate(specs):
            co, ci, taps = sp['shape']
            f = np.asarray(sp['rows'], dtype=bool)
            if f.shape != (co,):
                raise ValueError(f'kml: layer {k} has {co} rows, its flags the shape {f.shape}')
            idx = np.flatnonzero(f).astype(np.int32)
            rg = int(_lib.lib.rick_kml_rows_per_group(ci, taps))
            ng = (len(idx) + rg - 1) // rg
            L = rec[k]
            L.off, L.a_off, L.b_off, L.part_off = int(sp['off']), int(sp['a_off']), int(sp['b_off']), part
            L.co, L.ci, L.taps = co, ci, taps
            L.rows_off, L.nrows, L.rg, L.ngroups = sum(len(r) for r in rows), len(idx), rg, ng
            L.flags_off = sum(len(x) for x in flags)
            part += ng * rank * ci
            rows.append(idx)
            flags.append(f.astype(np.uint8))
            blocks.extend((k, g) for g in range(ng))
        self.rank, self.nlayers, self.layers_host = rank, len(specs), rec
        self.nrows_total = int(sum(len(r) for r in rows))
        self.nblocks, self.npart = len(blocks), part
        self.elements = int(sum(len(r) * sp['shape'][1] * sp['shape'][2] for r, sp in zip(rows, specs)))      # modulated elements
        self.max_co = max(sp['shape'][0] for sp in specs)
        self.max_ci = max(sp['shape'][1] for sp in specs)
        self.nflags = int(sum(len(x) for x in flags))
        if torch.device(device).type != 'cuda':
            return
        raw = np.frombuffer(ctypes.string_at(ctypes.addressof(rec), ctypes.sizeof(rec)), dtype=np.uint8).copy()
        self.layers_dev = torch.from_numpy(raw).to(device)
        self.rows_dev = torch.from_numpy(np.concatenate(rows + [np.zeros(1, np.int32)])).to(device)
        self.blocks_dev = torch.tensor(blocks + [(0, 0)], dtype=torch.int32).reshape(-1).to(device)
        self.flags_dev = torch.from_numpy(np.concatenate(flags)).to(device)


def _flat_f32(what, *tensors):
    dev = tensors[0].device
    for t in tensors:
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1) or t.device != dev:
            raise ValueError(f'kml: {what} must be dense 1-D float32 tensors on one HIP device')


def apply_tables(w0, w, fac, tables):
    """rick_kml_apply_f32 on raw buffers: W^ into the flagged rows of `w` (the layout of `w0`), from `w0` and the factors."""
    _flat_f32('w0, w and fac', w0, w, fac)
    if w.numel() != w0.numel():
        raise ValueError('kml: w and w0 must have one length')
    if tables.nblocks == 0:
        return
    from .op.conv import hbm_launch
    with torch.cuda.device(w0.device):
        _lib.check(hbm_launch('kml_apply', 8 * tables.elements, _lib.lib.rick_kml_apply_f32, _lib.ptr(w0), _lib.ptr(w), w0.numel(),
                              _lib.ptr(fac), fac.numel(), tables.rank, _lib.ptr(tables.layers_dev), tables.nlayers,
                              _lib.ptr(tables.rows_dev), tables.nrows_total, _lib.ptr(tables.blocks_dev), tables.nblocks,
                              _lib.stream_ptr()), 'rick_kml_apply_f32')


def grad_tables(grad, w0, fac, dfac, partials, tables):
    """rick_kml_grad_f32 + rick_kml_grad_finish_f32 on raw buffers: da / db of every layer into `dfac` (the layout of `fac`).
    partials: fp32 workspace of at least tables.npart entries."""
    _flat_f32('grad, w0, fac, dfac and partials', grad, w0, fac, dfac, partials)
    if grad.numel() != w0.numel() or fac.numel() != dfac.numel() or partials.numel() < tables.npart:
        raise ValueError('kml: grad / w0 and fac / dfac must pair up, partials must hold tables.npart entries')
    from .op.conv import hbm_launch
    with torch.cuda.device(w0.device):
        if tables.nblocks:
            _lib.check(hbm_launch('kml_grad', 8 * tables.elements, _lib.lib.rick_kml_grad_f32, _lib.ptr(grad), _lib.ptr(w0),
                                  w0.numel(), _lib.ptr(fac), _lib.ptr(dfac), fac.numel(), _lib.ptr(partials), tables.npart, tables.rank,
                                  _lib.ptr(tables.layers_dev), tables.nlayers, _lib.ptr(tables.rows_dev), tables.nrows_total,
                                  _lib.ptr(tables.blocks_dev), tables.nblocks, tables.max_ci, _lib.stream_ptr()), 'rick_kml_grad_f32')
        _lib.check(_lib.lib.rick_kml_grad_finish_f32(_lib.ptr(partials), tables.npart, _lib.ptr(dfac), fac.numel(),
                                                     _lib.ptr(tables.flags_dev), tables.nflags, tables.rank,
                                                     _lib.ptr(tables.layers_dev), tables.nlayers, tables.max_co, tables.max_ci,
                                                     _lib.stream_ptr()), 'rick_kml_grad_finish_f32')


class KmlState:
    """The KML adapter over the optimised slice ``[flat.lo:flat.hi]`` of a FlatParams.

    flat: the FlatParams.  rank: R, 1 ... 8, the same for all layers.  names: the modulated parameters (default: every parameter
    of the slice with ``dim() >= 4``).  generator: the torch.Generator b ~ N(0, 1) is drawn with, on the CPU, in the order of
    `names` (None: the global CPU generator).  lr / betas: of the adapter's own Adam.

    Owns W0 (``w0``: fp32, the slice's layout, zero in the padding and on rows that were never flagged), the factors (``a[name]``,
    ``b[name]``: nn.Parameters inside ``fac``, a FlatParams), their optimiser (``optim``), the row flags (``rows[name]``: bool
    [co]) and, on the device, the layer table, the compacted row lists and the db partials."""

    def __init__(self, flat, rank, names=None, generator=None, lr=0.002, betas=(0.0, 0.99)):
        from .train import FlatParams, MaskedFlatAdam
        if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= MAX_RANK:
            raise ValueError(f'kml: rank must be an integer in 1 ... {MAX_RANK}, got {rank!r}')
        self.flat, self.rank = flat, rank
        self.lo, self.hi = flat.lo, flat.hi
        self.n = self.hi - self.lo
        self.device = flat.flat.device
        owned = [flat.names[i] for i in flat.opt_idx]
        if names is None:
            names = [n for n in owned if flat.params[flat.index[n]].dim() >= 4]
        names = list(names)
        if not names:
            raise ValueError('kml: no parameter to modulate')
        if len(set(names)) != len(names):
            raise ValueError('kml: a name is listed twice')
        for n in names:
            if n not in flat.index:
                raise KeyError(f'kml: the FlatParams has no parameter {n}')
            if n not in owned:
                raise ValueError(f'kml: {n} lies outside the optimised slice')
        self.names = names
        self.shape3 = {n: _view3(flat.params[flat.index[n]]) for n in names}
        if max(ci for _, ci, _ in self.shape3.values()) * rank > 16384:
            raise ValueError('kml: ci * rank must not exceed 16384 (the gradient kernel keeps a layer\'s db in 64 KB of LDS)')
        self.w0 = torch.zeros(self.n, device=self.device, dtype=torch.float32)
        named = []
        for n in names:
            named.append((f'a.{n}', nn.Parameter(torch.zeros(self.shape3[n][0], rank, device=self.device))))
        for n in names:
            bn = torch.randn(self.shape3[n][1], rank, generator=generator, dtype=torch.float32)
            named.append((f'b.{n}', nn.Parameter(bn.to(self.device))))
        self.fac = FlatParams(named)
        self.a = {n: self.fac.params[self.fac.index[f'a.{n}']] for n in names}
        self.b = {n: self.fac.params[self.fac.index[f'b.{n}']] for n in names}
        for p in self.fac.params:
            p._rick_group = _NoPack
        self.optim = MaskedFlatAdam(self.fac, lr, tuple(betas))
        self.rows = {n: torch.zeros(self.shape3[n][0], dtype=torch.bool, device=self.device) for n in names}
        self._build_tables()

    # ---- layout
    def segment(self, name):
        """[start, end) of a parameter inside ``w0`` (and inside ``flat.flat[lo:hi]`` / ``flat.grad[lo:hi]``)."""
        lo, hi = self.flat.segment(name)
        return lo - self.lo, hi - self.lo

    def _w3(self, buf, name):
        a, b = self.segment(name)
        return buf[a:b].view(self.shape3[name])

    def weight(self, name):
        """The live weight as a [co, ci, taps] view of the flat parameter buffer."""
        return self._w3(self.flat.flat[self.lo:self.hi], name)

    def grad(self, name):
        return self._w3(self.flat.grad[self.lo:self.hi], name)

    def snapshot(self, name):
        return self._w3(self.w0, name)

    def modulation(self, name):
        """1 + a b^T, [co, ci] (fp32; every row, flagged or not)."""
        return 1.0 + self.a[name].detach() @ self.b[name].detach().t()

    @property
    def flagged(self):
        return self.nrows_total

    # ---- tables
    def _build_tables(self):
        specs = [dict(off=self.segment(n)[0], a_off=int(self.fac.offsets[self.fac.index[f'a.{n}']]),
                      b_off=int(self.fac.offsets[self.fac.index[f'b.{n}']]), shape=self.shape3[n], rows=self.rows[n].cpu().numpy())
                 for n in self.names]
        t = self.tables = KmlTables(specs, self.rank, self.device)
        self.nrows_total, self.nblocks, self.elements = t.nrows_total, t.nblocks, t.elements
        if self.w0.is_cuda and (getattr(self, 'partials', None) is None or self.partials.numel() < max(1, t.npart)):
            self.partials = torch.zeros(max(1, t.npart), device=self.device, dtype=torch.float32)

    def _check_rows(self, rows, what):
        out = {}
        for n, f in rows.items():
            if n not in self.rows:
                raise KeyError(f'kml: {what} names {n}, which is not a modulated parameter')
            f = torch.as_tensor(f)
            if f.dtype != torch.bool or tuple(f.shape) != (self.shape3[n][0],):
                raise ValueError(f'kml: {what}[{n}] must be a bool tensor of shape ({self.shape3[n][0]},), got {f.dtype} '
                                 f'{tuple(f.shape)}')
            out[n] = f.to(self.device)
        return out

    def set_rows(self, rows):
        """rows: {name: bool[co]}; a name that is not given keeps its flags.  A row that ENTERS takes W0[o] := the live weight row,
        a[o, :] := 0 and zero Adam moments of a[o, :]; a row that LEAVES keeps its current W^ as an ordinary weight (nothing is
        written to it); b persists.  The tables are rebuilt.  Validated completely before anything is touched."""
        rows = self._check_rows(rows, 'set_rows')
        with torch.no_grad():
            for n, f in rows.items():
                enter = f & ~self.rows[n]
                if bool(enter.any()):
                    self.snapshot(n)[enter] = self.weight(n)[enter]
                    ai = self.fac.index[f'a.{n}']
                    lo = int(self.fac.offsets[ai])
                    hi = lo + self.fac.sizes[ai]
                    for buf in (self.fac.flat, self.optim.m, self.optim.v):
                        buf[lo:hi].view(-1, self.rank)[enter] = 0
                self.rows[n] = f.clone()
        self._build_tables()

    # ---- the two passes
    def grads_(self):
        """a.grad, b.grad (the adapter's flat gradient buffer) from flat.grad and W0.  No host synchronisation.  With no row
        flagged only the finishing launch runs (it writes the zeros)."""
        if not self.w0.is_cuda:
            return self._grads_cpu()
        grad_tables(self.flat.grad[self.lo:self.hi], self.w0, self.fac.flat, self.fac.grad, self.partials, self.tables)

    def apply_(self):
        """W^ into the flagged rows of the flat parameter buffer; then the packed weights of the network go stale."""
        from . import op
        if not self.w0.is_cuda:
            self._apply_cpu()
        else:
            apply_tables(self.w0, self.flat.flat[self.lo:self.hi], self.fac.flat, self.tables)
        op.bump_weights_epoch(self.flat.params)

    def adam_step(self):
        """One step of the adapter's own Adam on a.grad / b.grad (device tensors only: it is rick_masked_adam_dev_f32)."""
        self.optim.step()

    def step(self):
        self.grads_()
        self.adam_step()
        self.apply_()

    # ---- the same definition from torch ops in fp64 (CPU tensors)
    def _grads_cpu(self):
        with torch.no_grad():
            self.fac.grad.zero_()
            for n in self.names:
                f = self.rows[n]
                if not bool(f.any()):
                    continue
                P = (self.grad(n).double() * self.snapshot(n).double()).sum(2) * f.double()[:, None]
                self.a[n].grad.copy_(P @ self.b[n].detach().double())
                self.b[n].grad.copy_(P.t() @ self.a[n].detach().double())

    def _apply_cpu(self):
        with torch.no_grad():
            for n in self.names:
                f = self.rows[n]
                if not bool(f.any()):
                    continue
                m = 1.0 + self.a[n].detach().double() @ self.b[n].detach().double().t()
                self.weight(n)[f] = (self.snapshot(n).double() * m[:, :, None]).to(torch.float32)[f]

    # ---- persistence
    def state_dict(self):
        """Copies: 'w0.<name>', 'a.<name>', 'b.<name>' (the parameter's / factors' shapes), 'rows.<name>' (bool [co]), the Adam
        moments 'm.a.<name>', 'v.a.<name>', 'm.b.<name>', 'v.b.<name>' and 'steps' (int64, one count per factor tensor in the
        order a.*, b.*)."""
        out = {}
        for n in self.names:
            p = self.flat.params[self.flat.index[n]]
            a, b = self.segment(n)
            out[f'w0.{n}'] = self.w0[a:b].clone().view(p.shape)
            out[f'rows.{n}'] = self.rows[n].clone()
            for key in ('a', 'b'):
                i = self.fac.index[f'{key}.{n}']
                lo = int(self.fac.offsets[i])
                hi = lo + self.fac.sizes[i]
                shape = self.fac.params[i].shape
                out[f'{key}.{n}'] = self.fac.flat[lo:hi].clone().view(shape)
                out[f'm.{key}.{n}'] = self.optim.m[lo:hi].clone().view(shape)
                out[f'v.{key}.{n}'] = self.optim.v[lo:hi].clone().view(shape)
        out['steps'] = torch.tensor(self.optim.steps, dtype=torch.int64)
        return out

    def load_state_dict(self, state):
        """The inverse of state_dict().  Everything is validated and staged before anything live is touched; then copied IN PLACE
        (w0, the factors and the moments keep their memory) and the tables are rebuilt.  The flat parameter buffer is not
        written: call apply_() to re-impose W^."""
        staged = []

        def take(key, shape, dtype, dst):
            if key not in state:
                raise KeyError(f'kml: the state has no entry {key}')
            t = state[key]
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
                raise ValueError(f'kml: {key} has shape {tuple(getattr(t, "shape", ()))}, expected {tuple(shape)}')
            if t.dtype != dtype:
                raise ValueError(f'kml: {key} has dtype {t.dtype}, expected {dtype}')
            if dtype != torch.bool and t.is_floating_point() and not bool(torch.isfinite(t).all()):
                raise ValueError(f'kml: {key} has a non-finite entry')
            staged.append((dst, t.detach().reshape(-1).to(self.device)))

        rows = {}
        for n in self.names:
            p = self.flat.params[self.flat.index[n]]
            a, b = self.segment(n)
            take(f'w0.{n}', p.shape, torch.float32, self.w0[a:b])
            take(f'rows.{n}', (self.shape3[n][0],), torch.bool, None)
            rows[n] = staged.pop()[1]
            for key in ('a', 'b'):
                i = self.fac.index[f'{key}.{n}']
                lo = int(self.fac.offsets[i])
                hi = lo + self.fac.sizes[i]
                shape = self.fac.params[i].shape
                take(f'{key}.{n}', shape, torch.float32, self.fac.flat[lo:hi])
                take(f'm.{key}.{n}', shape, torch.float32, self.optim.m[lo:hi])
                take(f'v.{key}.{n}', shape, torch.float32, self.optim.v[lo:hi])
        take('steps', (len(self.optim.steps),), torch.int64, None)
        steps = [int(s) for s in staged.pop()[1].cpu()]
        if min(steps) < 0:
            raise ValueError('kml: steps has a negative entry')
        with torch.no_grad():
            for dst, src in staged:
                dst.copy_(src)
        for n in self.names:
            self.rows[n] = rows[n].clone()
        self.optim.steps[:] = steps
        self.optim.sync_steps_to_device()
        self._build_tables()
