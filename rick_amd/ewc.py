"""Elastic weight consolidation (Li et al., "Few-shot Image Generation with Elastic Weight Consolidation", NeurIPS 2020) on the
flat parameter buffers: the penalty

    L_ewc = sum_i F_i (theta_i - theta*_i)^2            d(weight L_ewc) / d theta_i = 2 weight F_i (theta_i - theta*_i)

over the optimised slice of a ``FlatParams``, with theta* the source model's weights and F their Fisher information.

    fisher = estimate_fisher(g_source_copy, d_source_copy, latents)      # the paper's estimate on the source pair
    anchor = EwcAnchor(trainer.g_flat, source_state, fisher)             # or trainer.set_ewc(source_state, fisher)
    value = penalty_(anchor, weight, mask)                               # flat.grad += the gradient term; returns sum (fp64)

``fisher=None`` gives F = 1 on every parameter: the L2-SP penalty ("Explicit Inductive Bias for Transfer Learning with
Convolutional Networks", Li et al., 2018), by the same code.

On the device ``penalty_`` is two launches of rick_amd/csrc/ewc.hip (include/rick_hip.h "EWC"): one pass over theta, theta*, F
and the gradient with three fp32 roundings per gradient element, the value summed in fp64 in a fixed order (bit-identical from run
to run), no temporaries and no autograd node; every buffer it touches belongs to the anchor or the FlatParams, so the launches can
be captured in a step graph.  CPU tensors take the same definition composed from torch ops in fp64.  Elements the optimiser's
mask freezes or prunes (``mask & 3``) neither pull nor count.
"""
import math

import torch

from . import _lib
from .adapter import FlatSlice
from .flat import FisherAccumulator


def _same_device(a, b):
    return a.type == b.type and (a.type != 'cuda' or (a.index or 0) == (b.index or 0))


class EwcAnchor(FlatSlice):
    """theta* and F of the optimised slice ``[flat.lo:flat.hi]`` of a FlatParams as two fp32 buffers in the slice's own layout:
    the same offsets, zero in the padding between parameters (a padding element adds F (0 - 0)^2 = 0).

    flat: the FlatParams.  source_state: {name: tensor} with an entry for every optimised parameter (a source generator's
    ``state_dict()``; other entries are ignored).  fisher: {name: tensor} likewise, every entry finite and >= 0, or None for
    all ones.  Tensors must have the parameter's shape and lie on the FlatParams' device; they are read as fp32.

    The anchor also owns the fp64 partial sums and the result of ``penalty_`` (allocated here, once)."""

    def __init__(self, flat, source_state, fisher=None):
        super().__init__(flat)
        self.names = self.owned
        self.anchor = self._stage(source_state, 'source_state', False)
        self.fisher = self._stage(fisher, 'fisher', True)
        self.blocks = int(_lib.lib.rick_ewc_blocks(self.n))
        self.partials = torch.zeros(max(1, self.blocks), device=self.device, dtype=torch.float64)
        self.value = torch.zeros((), device=self.device, dtype=torch.float64)

    def _stage(self, mapping, what, is_fisher):
        """A new buffer in the slice's layout filled from `mapping` — validated completely before anything live is touched."""
        buf = torch.zeros(self.n, device=self.device, dtype=torch.float32)
        for name in self.names:
            a, b = self.segment(name)
            if mapping is None:
                buf[a:b].fill_(1.0)
                continue
            if name not in mapping:
                raise KeyError(f'EwcAnchor: {what} has no entry for {name}')
            t = mapping[name]
            shape = tuple(self.flat.params[self.flat.index[name]].shape)
            if not torch.is_tensor(t) or tuple(t.shape) != shape:
                raise ValueError(f'EwcAnchor: {what}[{name}] has shape {tuple(getattr(t, "shape", ()))}, the parameter {shape}')
            if not _same_device(t.device, self.device):
                raise ValueError(f'EwcAnchor: {what}[{name}] is on {t.device}, the parameters on {self.device}')
            buf[a:b].copy_(t.detach().reshape(-1))
        if is_fisher and mapping is not None and not bool((torch.isfinite(buf) & (buf >= 0)).all()):
            for name in self.names:                        # one reduction in the good case; name the offender in the bad one
                a, b = self.segment(name)
                if not bool((torch.isfinite(buf[a:b]) & (buf[a:b] >= 0)).all()):
                    raise ValueError(f'EwcAnchor: {what}[{name}] has a negative or non-finite entry')
        return buf

    def state_dict(self):
        """{'anchor.<name>': theta*, 'fisher.<name>': F} — copies, in the parameters' shapes."""
        out = {}
        for key, buf in (('anchor', self.anchor), ('fisher', self.fisher)):
            for name in self.names:
                a, b = self.segment(name)
                out[f'{key}.{name}'] = buf[a:b].clone().view(self.flat.params[self.flat.index[name]].shape)
        return out

    def load_state_dict(self, state):
        """The inverse of state_dict(), with the constructor's checks.  Copies IN PLACE: captured launches keep reading the same
        memory, so the next replay of a step graph sees the new values."""
        staged = [self._stage({n: state[f'{key}.{n}'] for n in self.names if f'{key}.{n}' in state}, key, key == 'fisher')
                  for key in ('anchor', 'fisher')]
        self.anchor.copy_(staged[0])
        self.fisher.copy_(staged[1])


def accumulate_(theta, anchor, fisher, grad, weight, mask=None, partials=None, out=None):
    """The penalty on four flat fp32 tensors of one length n (and an optional uint8 mask of n): grad += 2 weight F (theta - theta*)
    on the unmasked elements, in place; returns sum F (theta - theta*)^2 over them as a 0-dim fp64 tensor (`out`, when given).
    `partials`: fp64 workspace of at least rick_ewc_blocks(n) entries (device tensors; allocated when not given)."""
    n = theta.numel()
    weight = float(weight)
    if weight < 0 or not math.isfinite(weight):
        raise ValueError(f'ewc: weight must be finite and >= 0, got {weight}')
    for t in (theta, anchor, fisher, grad):
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or t.device != theta.device or (n > 1 and t.stride(0) != 1):
            raise ValueError('ewc: theta, anchor, fisher and grad must be dense 1-D float32 tensors of one length on one device')
    if mask is not None and (mask.dtype != torch.uint8 or mask.dim() != 1 or mask.numel() != n or mask.device != theta.device
                             or (n > 1 and mask.stride(0) != 1)):
        raise ValueError('ewc: mask must be a dense uint8 tensor of the same length on the same device')
    if out is None:
        out = torch.zeros((), device=theta.device, dtype=torch.float64)
    if not theta.is_cuda:
        # the same definition in fp64: the fp32 difference d (as the kernel forms it), then everything in double
        keep = torch.ones(n, dtype=torch.bool) if mask is None else (mask & 3) == 0
        d = (theta - anchor).double()
        f = fisher.double()
        grad.copy_(torch.where(keep, (grad.double() + 2.0 * weight * f * d).to(torch.float32), grad))
        out.copy_(torch.where(keep, f * d * d, torch.zeros((), dtype=torch.float64)).sum())
        return out
    blocks = int(_lib.lib.rick_ewc_blocks(n))
    if partials is None:
        partials = torch.empty(max(1, blocks), device=theta.device, dtype=torch.float64)
    if partials.dtype != torch.float64 or partials.numel() < max(1, blocks) or partials.device != theta.device:
        raise ValueError('ewc: partials must hold rick_ewc_blocks(n) float64 entries on the same device')
    from .op.conv import hbm_launch
    with torch.cuda.device(theta.device):
        if n:
            _lib.check(hbm_launch('ewc', (20 + (mask is not None)) * n, _lib.lib.rick_ewc_f32, _lib.ptr(theta), _lib.ptr(anchor),
                                  _lib.ptr(fisher), _lib.ptr(grad), _lib.ptr(mask), n, weight, _lib.ptr(partials),
                                  _lib.stream_ptr()), 'rick_ewc_f32')
        _lib.check(_lib.lib.rick_ewc_finish_f64(_lib.ptr(partials), blocks, _lib.ptr(out), _lib.stream_ptr()), 'rick_ewc_finish_f64')
    return out


def penalty_(anchor, weight, mask=None):
    """``accumulate_`` on ``flat.flat[lo:hi]`` and ``flat.grad[lo:hi]`` of the anchor's FlatParams: adds the weighted gradient term
    into the flat gradient in place and returns the UNWEIGHTED sum, the anchor's own 0-dim fp64 tensor (rewritten by the next
    call).  mask: uint8 over the slice (the optimiser's ``mask[lo:hi]``) or None.  No allocation: safe inside a graph capture."""
    flat = anchor.flat
    return accumulate_(flat.flat[anchor.lo:anchor.hi], anchor.anchor, anchor.fisher, flat.grad[anchor.lo:anchor.hi], weight,
                       mask=mask, partials=anchor.partials, out=anchor.value)


def estimate_fisher(generator, discriminator, latents, fixed_noise=False):
    """The EWC paper's Fisher estimate on a (source) generator / discriminator pair: per latent, at batch 1, the gradient of
    ``g_nonsaturating_loss(D(G([z])))`` with respect to the generator's optimised parameters (``g_optim_filter``), squared and
    summed on the device (FisherAccumulator -> rick_sq_accumulate_f32, one fused multiply-add per sample and element), then
    divided by the number of latents.  Returns {name: tensor} in the parameters' shapes.  latents: an iterable of [512] or
    [1, 512] tensors.  fixed_noise: use the generator's stored noise maps instead of fresh draws.

    Every ``requires_grad`` flag it changes (the generator's other parameters and the discriminator's are switched off for the
    passes) is restored; RickTrainer.fisher_sweep and its masks are not involved."""
    from torch import autograd

    from .train import g_nonsaturating_loss, g_optim_filter
    latents = list(latents)
    if not latents:
        raise ValueError('estimate_fisher: needs at least one latent')
    named = [(n, p) for n, p in generator.named_parameters() if g_optim_filter(n)]
    owned = {id(p) for _, p in named}
    every = list(generator.parameters()) + list(discriminator.parameters())
    flags = [p.requires_grad for p in every]
    try:
        for p in every:
            p.requires_grad = id(p) in owned
        acc = FisherAccumulator(named)
        params = [p for _, p in named]
        for z in latents:
            fake, _ = generator([z.view(1, -1)], randomize_noise=not fixed_noise)
            fake_pred, _ = discriminator(fake)
            acc.add(autograd.grad(g_nonsaturating_loss(fake_pred), params, allow_unused=True))
    finally:
        for p, f in zip(every, flags):
            p.requires_grad = f
    # the mean: a division in fp64 rounded once to fp32 (a multiplication by fl32(1 / count) would round twice)
    return {n: v.copy_(v.double().div_(len(latents))) for n, v in acc.acc.items()}
