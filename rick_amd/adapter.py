"""What the features on the flat parameter buffers share.  FlatSlice: the optimised slice ``[flat.lo:flat.hi]`` of a FlatParams
and buffers in its layout (EWC's anchor).  FlatAdapter: a slice whose weights are REWRITTEN from a snapshot W0 and learnt factors
(KML, FSGAN's singular values): which parameters, their [co, ci, taps] views, the factors in a FlatParams of their own with their
own MaskedFlatAdam, the grads_ / adam_step / apply_ bracket around the network's optimiser step, and the state_dict round trip.

    adapter.grads_()                                       # the factors' gradients from flat.grad
    ... the network's masked Adam (the freeze bit leaves the adapted weights alone) ...
    adapter.adam_step(); adapter.apply_()                  # or adapter.step() = grads_, adam_step, apply_

A subclass sets ``w0`` (fp32, the slice's layout), calls ``_own_factors`` and supplies ``_grads_dev`` / ``_apply_dev`` (its
launches), ``_grads_cpu`` / ``_apply_cpu`` (the same definition from torch ops in fp64) and ``_entries``."""
import ctypes

import numpy as np
import torch
from torch import nn

from . import op
from .flat import FlatParams, MaskedFlatAdam


class _NoPack:
    """Stands in for a PackGroup on the factors: MaskedFlatAdam.step reports the parameters it updated to op.bump_weights_epoch,
    which invalidates EVERY packed weight when one of them belongs to no group — the factors are never packed."""
    epoch = 0


def _view3(p, tag):
    """(co, ci, taps) of a weight tensor."""
    shape = tuple(p.shape)
    if len(shape) == 5:
        if shape[0] != 1:
            raise ValueError(f'{tag}: a 5-D weight needs a leading dim of 1, got {shape}')
        shape = shape[1:]
    if len(shape) < 2:
        raise ValueError(f'{tag}: a weight needs at least two dims, got {shape}')
    return shape[0], shape[1], int(np.prod(shape[2:], dtype=np.int64))


def flat_f32(tag, what, *tensors):
    dev = tensors[0].device
    for t in tensors:
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1) or t.device != dev:
            raise ValueError(f'{tag}: {what} must be dense 1-D float32 tensors on one HIP device')


def upload_table(rec, device):
    """A ctypes array of layer records as a byte tensor on `device`."""
    raw = np.frombuffer(ctypes.string_at(ctypes.addressof(rec), ctypes.sizeof(rec)), dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device)


class FlatSlice:
    """The optimised slice of a FlatParams: ``flat``, ``lo``, ``hi``, ``n`` = hi - lo, ``device`` and ``owned``, the names of its
    parameters in registration order."""

    def __init__(self, flat):
        self.flat = flat
        self.lo, self.hi = flat.lo, flat.hi
        self.n = self.hi - self.lo
        self.device = flat.flat.device
        self.owned = [flat.names[i] for i in flat.opt_idx]

    def segment(self, name):
        """[start, end) of a parameter inside a buffer of the slice's layout (and inside ``flat.flat[lo:hi]`` / ``flat.grad[lo:hi]``)."""
        lo, hi = self.flat.segment(name)
        return lo - self.lo, hi - self.lo


class FlatAdapter(FlatSlice):
    """names: the adapted parameters (None: every parameter of the slice that `default` accepts).  tag: the prefix of every
    message.  Sets ``names`` and ``shape3`` ({name: (co, ci, taps)}); everything is validated before anything is built."""

    def __init__(self, flat, names, tag, default):
        super().__init__(flat)
        self.tag = tag
        if names is None:
            names = [n for n in self.owned if default(flat.params[flat.index[n]])]
        names = list(names)
        if not names:
            raise ValueError(f'{tag}: no parameter to adapt')
        if len(set(names)) != len(names):
            raise ValueError(f'{tag}: a name is listed twice')
        for n in names:
            if n not in flat.index:
                raise KeyError(f'{tag}: the FlatParams has no parameter {n}')
            if n not in self.owned:
                raise ValueError(f'{tag}: {n} lies outside the optimised slice')
        self.names = names
        self.shape3 = {n: _view3(flat.params[flat.index[n]], tag) for n in names}

    # ---- views
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

    # ---- the learnt factors
    def _own_factors(self, named, lr, betas):
        """``fac``: a FlatParams of the factors [(key, nn.Parameter)]; ``optim``: their MaskedFlatAdam."""
        self.fac = FlatParams(named)
        for p in self.fac.params:
            p._rick_group = _NoPack
        self.optim = MaskedFlatAdam(self.fac, lr, tuple(betas))

    def fac_range(self, key):
        """(lo, hi, shape) of a factor inside ``fac.flat`` / ``fac.grad`` / ``optim.m`` / ``optim.v``."""
        i = self.fac.index[key]
        lo = int(self.fac.offsets[i])
        return lo, lo + self.fac.sizes[i], tuple(self.fac.params[i].shape)

    # ---- the step
    def grads_(self):
        """The factors' gradients (``fac.grad``) from flat.grad.  No host synchronisation."""
        if self.w0.is_cuda:
            self._grads_dev()
        else:
            self._grads_cpu()

    def apply_(self):
        """W^ into the adapted weights of the flat parameter buffer; then the packed weights of the network go stale."""
        if self.w0.is_cuda:
            self._apply_dev()
        else:
            self._apply_cpu()
        op.bump_weights_epoch(self.flat.params)

    def adam_step(self):
        """One step of the adapter's own Adam on ``fac.grad`` (device tensors only: it is rick_masked_adam_dev_f32)."""
        self.optim.step()

    def step(self):
        self.grads_()
        self.adam_step()
        self.apply_()

    # ---- persistence
    def _entries(self):
        """(key, shape, dtype, live tensor or None) of every tensor of the state but 'steps', in a fixed order.  None: the entry
        has no buffer to be copied into; its checked value goes to ``_loaded``."""
        raise NotImplementedError

    def _loaded(self, extra):
        """The end of load_state_dict.  extra: {key: tensor on the device} of the entries without a live tensor."""

    def state_dict(self):
        """Copies of every live tensor of ``_entries()`` in its shape, and 'steps' (int64, one count per factor tensor)."""
        out = {key: dst.detach().clone().view(shape) for key, shape, _, dst in self._entries() if dst is not None}
        out['steps'] = torch.tensor(self.optim.steps, dtype=torch.int64)
        return out

    def load_state_dict(self, state):
        """The inverse of state_dict().  Everything is validated and staged before anything live is touched; then copied IN PLACE
        (w0, the factors and the moments keep their memory).  The flat parameter buffer is not written: call apply_() to
        re-impose W^."""
        staged, extra = [], {}
        for key, shape, dtype, dst in self._entries() + [('steps', (len(self.optim.steps),), torch.int64, None)]:
            if key not in state:
                raise KeyError(f'{self.tag}: the state has no entry {key}')
            t = state[key]
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape):
                raise ValueError(f'{self.tag}: {key} has shape {tuple(getattr(t, "shape", ()))}, expected {tuple(shape)}')
            if t.dtype != dtype:
                raise ValueError(f'{self.tag}: {key} has dtype {t.dtype}, expected {dtype}')
            if t.is_floating_point() and not bool(torch.isfinite(t).all()):
                raise ValueError(f'{self.tag}: {key} has a non-finite entry')
            if dst is None:
                extra[key] = t.detach().to(self.device)
            else:
                staged.append((dst, t.detach().to(self.device)))
        steps = [int(s) for s in extra.pop('steps').cpu()]
        if min(steps) < 0:
            raise ValueError(f'{self.tag}: steps has a negative entry')
        with torch.no_grad():
            for dst, src in staged:
                dst.copy_(src.reshape(dst.shape))
        self.optim.steps[:] = steps
        self.optim.sync_steps_to_device()
        self._loaded(extra)
