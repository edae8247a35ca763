"""Dual contrastive losses (DCL, "A Closer Look at Few-shot Image Generation", Zhao, Ding, Huang, Cheung, CVPR 2022) on the
cross-Gram kernels of rick_amd/csrc/gram.hip: two InfoNCE terms that tie the networks being adapted to the frozen source
networks, one on generator features (CL1), one on discriminator features (CL2).

    feats_t, feats_s = trainer._feature_pair(z)                          # G_t with grad, frozen G_s without, same z and noise maps
    cl1 = generator_contrastive_loss(feats_t, feats_s, cdc.draw_layers(g.n_latent, B), tau)
    cl2 = discriminator_contrastive_loss(D_t feats of the fakes, D_s feats of G_s's images, D_t feats of the reals,
                                         draw_d_layers(len(feats), B), tau)

This docstring is the specification (no copy of the paper or its code was at hand; the weights the paper uses are recalled as
lambda1 = 2, lambda2 = 0.5 and are unverified):

    cos(u, v) = <u, v> / (max(|u|, eps) max(|v|, eps)),   eps = 1e-8, over all elements of one sample's feature map
    s(u, v)   = cos(u, v) / tau,   tau = 0.07

    CL1 = mean_i  -log softmax_j( s(G_t^{l_i}(z_i), G_s^{l_i}(z_j)) )[j = i],   j = 0 ... B - 1
          one layer l_i per sample (cdc.draw_layers); gradients flow into the target features only; B = 1 gives exactly 0.

    CL2 = mean_i  -log softmax( [ s(a_i, p_i), s(a_i, x_1), ..., s(a_i, x_M) ] )[0]
          anchor a_i = D_t^{l_i}(G_t(z_i)), positive p_i = D_s^{l_i}(G_s(z_i)) (same latents, mixing index and noise maps, frozen
          networks, no gradient), negatives x_j = D_t^{l_i}(real_j) for the M reals of the step.  Minimised in the D step: its
          gradient reaches D through the anchors and the negatives and reaches no generator.  l_i is uniform over the whole
          feature list Discriminator.forward returns (draw_d_layers).

Every cosine between two sets comes from ``xgram(a, b)``: C = A B^T, na = |a_i|^2, nb = |b_j|^2 in fp64 from ONE pass over both
operands, one call per distinct drawn layer and operand pair.  On the device it runs rick_xgram_f32 (the summation order of
rick_gram_f32: every entry is bit-identical to ``cdc.gram`` of the same two rows, identical from run to run, and depends on its
two rows alone) and its backward pass dA = gC B + 2 diag(gna) A runs rick_xrowmix_f32 (dB: the same call with the roles swapped,
launched only when b needs a gradient).  The operands are read where they lie: two tensors, or two halves ``f[:B]``, ``f[B:]``
of one, in any memory layout the two share.  CPU tensors, and row counts above 8, take a torch composition that accumulates in
fp64.  Everything after the products is [B, B] fp64 tensor work.
"""
import numpy as np
import torch

from .cdc import EPS, MAX_B, _rows, _sample_dense

TAU = 0.07


def _use_kernels(a, b):
    return a.is_cuda and b.is_cuda and a.device == b.device and 1 <= a.shape[0] <= MAX_B and 1 <= b.shape[0] <= MAX_B


def _same_layout(a, b):
    """True if a sample of b lies in memory like a sample of a (the kernels pair the k-th value of a row with the k-th of another)."""
    return all(sa == sb for sa, sb, sz in zip(a.stride()[1:], b.stride()[1:], a.shape[1:]) if sz > 1)


def _xgram_rows(ra, rb):
    """rick_xgram_f32 on [Ba, n] and [Bb, n] fp32 device tensors with row stride n -> C [Ba, Bb], na [Ba], nb [Bb] fp64."""
    from . import _lib
    (Ba, n), Bb = ra.shape, rb.shape[0]
    out = torch.empty(Ba * Bb + Ba + Bb, device=ra.device, dtype=torch.float64)
    C, na, nb = out[:Ba * Bb].view(Ba, Bb), out[Ba * Bb:Ba * Bb + Ba], out[Ba * Bb + Ba:]
    with torch.cuda.device(ra.device):
        ws = torch.empty(_lib.lib.rick_xgram_workspace_bytes(Ba, Bb, n) // 4, device=ra.device, dtype=torch.float32)
        _lib.check(_lib.lib.rick_xgram_f32(ra.data_ptr(), Ba, rb.data_ptr(), Bb, n, ws.data_ptr(), C.data_ptr(), na.data_ptr(),
                                           nb.data_ptr(), _lib.stream_ptr()), 'rick_xgram_f32')
    return C, na, nb


def xrowmix(M, d, a, b, out=None):
    """y[k] = d[k] a[k] + sum_m M[k][m] b[m] on rick_xrowmix_f32: M [Ba, Bb], d [Ba], a [Ba, n], b [Bb, n] (row stride n) fp32 on
    one device, Ba, Bb <= 8; M and d are read from device memory (no host copy).  No autograd."""
    from . import _lib
    if a.dim() != 2 or b.dim() != 2:
        raise ValueError(f'dcl.xrowmix: a {tuple(a.shape)}, b {tuple(b.shape)}: expected [Ba, n] and [Bb, n]')
    (Ba, n), Bb = a.shape, b.shape[0]
    if out is None:
        out = torch.empty_like(a)
    for t in (M, d, a, b, out):
        if not t.is_cuda or t.dtype != torch.float32 or t.device != a.device:
            raise RuntimeError('dcl.xrowmix: float32 tensors on one device')
    if (tuple(M.shape) != (Ba, Bb) or tuple(d.shape) != (Ba,) or b.shape[1] != n or out.shape != a.shape
            or not 1 <= Ba <= MAX_B or not 1 <= Bb <= MAX_B or n < 1):
        raise ValueError(f'dcl.xrowmix: M {tuple(M.shape)}, d {tuple(d.shape)}, a {tuple(a.shape)}, b {tuple(b.shape)}, '
                         f'out {tuple(out.shape)}')
    for t in (a, b, out):
        if (t.shape[0] > 1 and t.stride(0) != n) or (n > 1 and t.stride(1) != 1):
            raise ValueError('dcl.xrowmix: a, b and out must have row stride n')
    M, d = M.contiguous(), d.contiguous()
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib.rick_xrowmix_f32(M.data_ptr(), d.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), Ba, Bb, n,
                                             _lib.stream_ptr()), 'rick_xrowmix_f32')
    return out


def _adjoint(gC, gn, x, other, kernels):
    """gC other + 2 diag(gn) x, dense in the layout of x."""
    gx = torch.empty_like(x)
    if kernels:
        xrowmix(gC.to(torch.float32).contiguous(), (2.0 * gn).to(torch.float32), _rows(x), _rows(other), out=_rows(gx))
    else:
        _rows(gx).copy_(gC.double() @ _rows(other).double() + 2.0 * gn.double()[:, None] * _rows(x).double())
    return gx


class _XGram(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ad, bd = a.detach(), b.detach()
        if not _sample_dense(ad):
            ad = ad.contiguous()
        if not _sample_dense(bd) or not _same_layout(ad, bd):            # b in the layout of a
            bd = torch.empty_strided(bd.shape, (ad[0].numel(),) + tuple(ad.stride()[1:]), dtype=bd.dtype, device=bd.device).copy_(bd)
        ra, rb = _rows(ad), _rows(bd)
        ctx.kernels = _use_kernels(ad, bd)
        if ctx.kernels:
            C, na, nb = _xgram_rows(ra, rb)
        else:
            a64, b64 = ra.double(), rb.double()
            C, na, nb = a64 @ b64.t(), (a64 * a64).sum(1), (b64 * b64).sum(1)
        ctx.save_for_backward(ad, bd)
        return C, na, nb

    @staticmethod
    def backward(ctx, gC, gna, gnb):
        if torch.is_grad_enabled():
            raise RuntimeError('dcl.xgram: the backward pass is first order only (create_graph=True is not supported)')
        ad, bd = ctx.saved_tensors
        ga = _adjoint(gC, gna, ad, bd, ctx.kernels) if ctx.needs_input_grad[0] else None
        gb = _adjoint(gC.t(), gnb, bd, ad, ctx.kernels) if ctx.needs_input_grad[1] else None
        return ga, gb


def xgram(a, b):
    """a [Ba, ...], b [Bb, ...] fp32 with equal sample shapes -> (C [Ba, Bb], na [Ba], nb [Bb]) fp64: C[i][j] = <a[i], b[j]>,
    na[i] = <a[i], a[i]>, nb[j] = <b[j], b[j]> over all elements of a sample.  Differentiable with respect to both operands, first
    order only (``create_graph=True`` raises in the backward pass); a gradient has its operand's layout.  Each sample must be one
    dense block of memory, in the same dimension order in both operands (contiguous, channels-last, views ``f[:B]`` / ``f[B:]`` of
    one tensor, ...); anything else is copied first."""
    for name, x in (('a', a), ('b', b)):
        if x.dim() < 1 or x.shape[0] < 1 or x[0].numel() < 1:
            raise ValueError(f'dcl.xgram: expected [B >= 1, ...] with at least one element per sample, got {name} {tuple(x.shape)}')
        if x.dtype != torch.float32:
            raise RuntimeError(f'dcl.xgram: features must be float32, got {name} {x.dtype}')
    if a.shape[1:] != b.shape[1:]:
        raise ValueError(f'dcl.xgram: sample shapes differ: a {tuple(a.shape)}, b {tuple(b.shape)}')
    if a.device != b.device:
        raise RuntimeError(f'dcl.xgram: a on {a.device}, b on {b.device}')
    return _XGram.apply(a, b)


def cross_cosine(a, b):
    """[Ba, Bb] fp64: cos(a[i], b[j]) of the module docstring (torch.nn.functional.cosine_similarity with its default eps, applied
    to the three products of one ``xgram``)."""
    C, na, nb = xgram(a, b)
    return C / (na.clamp_min(EPS * EPS).sqrt()[:, None] * nb.clamp_min(EPS * EPS).sqrt()[None, :])


def _check(feats, layers, B, who, what):
    for l in set(layers):
        if feats[l].shape[0] != B:
            raise ValueError(f'dcl.{who}: {what} layer {l} holds {feats[l].shape[0]} samples, expected {B}')


def generator_contrastive_loss(feats_t, feats_s, layers, tau=TAU):
    """CL1 of the module docstring: 0-dim fp32.  feats_t / feats_s: the feature lists of the generator being adapted and of the
    frozen source generator for the same latents; layers: one index per sample.  Gradients flow into feats_t only."""
    layers = [int(l) for l in layers]
    B = len(layers)
    if B < 1 or tau <= 0:
        raise ValueError('dcl.generator_contrastive_loss: needs at least one sample and tau > 0')
    _check(feats_t, layers, B, 'generator_contrastive_loss', 'target')
    _check(feats_s, layers, B, 'generator_contrastive_loss', 'source')
    terms = [None] * B
    for l in sorted(set(layers)):
        logp = torch.log_softmax(cross_cosine(feats_t[l], feats_s[l].detach()) / tau, 1)
        for i in range(B):
            if layers[i] == l:
                terms[i] = -logp[i, i]
    return torch.stack(terms).mean().to(torch.float32)


def discriminator_contrastive_loss(feats_fake_t, feats_fake_s, feats_real_t, layers, tau=TAU):
    """CL2 of the module docstring: 0-dim fp32.  feats_fake_t: features of the discriminator being adapted for the B fakes (the
    anchors); feats_fake_s: features of the frozen source discriminator for the source generator's images of the same latents (the
    positives, no gradient); feats_real_t: features of the discriminator being adapted for the M reals (the negatives); layers:
    one index per anchor.  Gradients flow into feats_fake_t and feats_real_t."""
    layers = [int(l) for l in layers]
    B = len(layers)
    if B < 1 or tau <= 0:
        raise ValueError('dcl.discriminator_contrastive_loss: needs at least one anchor and tau > 0')
    _check(feats_fake_t, layers, B, 'discriminator_contrastive_loss', 'anchor')
    _check(feats_fake_s, layers, B, 'discriminator_contrastive_loss', 'positive')
    terms = [None] * B
    for l in sorted(set(layers)):
        if feats_real_t[l].shape[0] < 1:
            raise ValueError(f'dcl.discriminator_contrastive_loss: layer {l} holds no negatives')
        pos = torch.diagonal(cross_cosine(feats_fake_t[l], feats_fake_s[l].detach()))          # [B]
        neg = cross_cosine(feats_fake_t[l], feats_real_t[l])                                   # [B, M]
        logp = torch.log_softmax(torch.cat([pos[:, None], neg], 1) / tau, 1)
        for i in range(B):
            if layers[i] == l:
                terms[i] = -logp[i, 0]
    return torch.stack(terms).mean().to(torch.float32)


def draw_d_layers(n_feats, batch, rng=None):
    """One discriminator feature per anchor, uniform over the whole list ``Discriminator.forward`` returns (14 entries at 256 px):
    ``randint(0, n_feats, size=batch)`` from ``rng`` (a numpy RandomState) or numpy's global state."""
    return (rng if rng is not None else np.random).randint(0, n_feats, size=batch)
