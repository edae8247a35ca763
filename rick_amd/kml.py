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
tensors take the same definition composed from torch ops in fp64.  Everything an adapter of the slice has in common — names,
views, the factors' own FlatParams and Adam, the step bracket, the state_dict round trip — is rick_amd/adapter.py's FlatAdapter."""
import numpy as np
import torch
from torch import nn

from . import _lib
from .adapter import FlatAdapter, flat_f32, upload_table

MAX_RANK = 8


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
        self.layers_dev = upload_table(rec, device)
        self.rows_dev = torch.from_numpy(np.concatenate(rows + [np.zeros(1, np.int32)])).to(device)
        self.blocks_dev = torch.tensor(blocks + [(0, 0)], dtype=torch.int32).reshape(-1).to(device)
        self.flags_dev = torch.from_numpy(np.concatenate(flags)).to(device)


def apply_tables(w0, w, fac, tables):
    """rick_kml_apply_f32 on raw buffers: W^ into the flagged rows of `w` (the layout of `w0`), from `w0` and the factors."""
    flat_f32('kml', 'w0, w and fac', w0, w, fac)
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
    flat_f32('kml', 'grad, w0, fac, dfac and partials', grad, w0, fac, dfac, partials)
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


class KmlState(FlatAdapter):
    """The KML adapter over the optimised slice ``[flat.lo:flat.hi]`` of a FlatParams.

    flat: the FlatParams.  rank: R, 1 ... 8, the same for all layers.  names: the modulated parameters (default: every parameter
    of the slice with ``dim() >= 4``).  generator: the torch.Generator b ~ N(0, 1) is drawn with, on the CPU, in the order of
    `names` (None: the global CPU generator).  lr / betas: of the adapter's own Adam.

    Owns W0 (``w0``: fp32, the slice's layout, zero in the padding and on rows that were never flagged), the factors (``a[name]``,
    ``b[name]``: nn.Parameters inside ``fac``, a FlatParams), their optimiser (``optim``), the row flags (``rows[name]``: bool
    [co]) and, on the device, the layer table, the compacted row lists and the db partials."""

    def __init__(self, flat, rank, names=None, generator=None, lr=0.002, betas=(0.0, 0.99)):
        if isinstance(rank, bool) or not isinstance(rank, int) or not 1 <= rank <= MAX_RANK:
            raise ValueError(f'kml: rank must be an integer in 1 ... {MAX_RANK}, got {rank!r}')
        super().__init__(flat, names, 'kml', lambda p: p.dim() >= 4)
        self.rank = rank
        if max(ci for _, ci, _ in self.shape3.values()) * rank > 16384:
            raise ValueError('kml: ci * rank must not exceed 16384 (the gradient kernel keeps a layer\'s db in 64 KB of LDS)')
        self.w0 = torch.zeros(self.n, device=self.device, dtype=torch.float32)
        named = [(f'a.{n}', nn.Parameter(torch.zeros(self.shape3[n][0], rank, device=self.device))) for n in self.names]
        for n in self.names:
            bn = torch.randn(self.shape3[n][1], rank, generator=generator, dtype=torch.float32)
            named.append((f'b.{n}', nn.Parameter(bn.to(self.device))))
        self._own_factors(named, lr, betas)
        self.a = {n: self.fac.params[self.fac.index[f'a.{n}']] for n in self.names}
        self.b = {n: self.fac.params[self.fac.index[f'b.{n}']] for n in self.names}
        self.rows = {n: torch.zeros(self.shape3[n][0], dtype=torch.bool, device=self.device) for n in self.names}
        self._build_tables()

    def modulation(self, name):
        """1 + a b^T, [co, ci] (fp32; every row, flagged or not)."""
        return 1.0 + self.a[name].detach() @ self.b[name].detach().t()

    @property
    def flagged(self):
        return self.nrows_total

    # ---- tables
    def _build_tables(self):
        specs = [dict(off=self.segment(n)[0], a_off=self.fac_range(f'a.{n}')[0], b_off=self.fac_range(f'b.{n}')[0],
                      shape=self.shape3[n], rows=self.rows[n].cpu().numpy()) for n in self.names]
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
                    lo, hi, _ = self.fac_range(f'a.{n}')
                    for buf in (self.fac.flat, self.optim.m, self.optim.v):
                        buf[lo:hi].view(-1, self.rank)[enter] = 0
                self.rows[n] = f.clone()
        self._build_tables()

    def set_rows_from_index_sets(self, freeze, zero):
        """set_rows with "frozen and not pruned" on every modulated layer: freeze / zero are {name: filter indices} or None (the
        index sets RICK's masks are built from); pruned filters are never modulated, a name in neither set flags nothing."""
        rows = {}
        for name in self.names:
            f = np.zeros(self.shape3[name][0], dtype=bool)
            if freeze is not None and name in freeze:
                f[np.asarray(freeze[name], dtype=np.int64)] = True
            if zero is not None and name in zero:
                f[np.asarray(zero[name], dtype=np.int64)] = False
            rows[name] = torch.from_numpy(f)
        self.set_rows(rows)

    # ---- the two passes.  With no row flagged only the finishing launch of grads_ runs (it writes the zeros).
    def _grads_dev(self):
        grad_tables(self.flat.grad[self.lo:self.hi], self.w0, self.fac.flat, self.fac.grad, self.partials, self.tables)

    def _apply_dev(self):
        apply_tables(self.w0, self.flat.flat[self.lo:self.hi], self.fac.flat, self.tables)

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

    # ---- persistence: 'w0.<name>', 'a.<name>', 'b.<name>' (the parameter's / factors' shapes), 'rows.<name>' (bool [co]), the Adam
    # moments 'm.a.<name>', 'v.a.<name>', 'm.b.<name>', 'v.b.<name>' and 'steps' (one count per factor tensor in the order a.*, b.*)
    def _entries(self):
        out = []
        for n in self.names:
            a, b = self.segment(n)
            out += [(f'w0.{n}', tuple(self.flat.params[self.flat.index[n]].shape), torch.float32, self.w0[a:b]),
                    (f'rows.{n}', (self.shape3[n][0],), torch.bool, None)]
            for key in (f'a.{n}', f'b.{n}'):
                lo, hi, shape = self.fac_range(key)
                out += [(key, shape, torch.float32, self.fac.flat[lo:hi]), (f'm.{key}', shape, torch.float32, self.optim.m[lo:hi]),
                        (f'v.{key}', shape, torch.float32, self.optim.v[lo:hi])]
        return out

    def state_dict(self):
        out = super().state_dict()
        out.update({f'rows.{n}': self.rows[n].clone() for n in self.names})
        return out

    def _loaded(self, extra):
        for n in self.names:
            self.rows[n] = extra[f'rows.{n}'].clone()
        self._build_tables()

