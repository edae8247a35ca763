"""Cross-domain distance-consistency loss (the structure-preserving regulariser of CDC, "Few-shot Image Generation via
Cross-domain Correspondence", Ojha et al., CVPR 2021) on the Gram kernels of rick_amd/csrc/gram.hip.

    feats_s = g_source([z], return_feats=True)[1]        # frozen source generator, no grad
    feats_t = g([z], return_feats=True)[1]               # the generator being adapted
    layers = draw_layers(g.n_latent, z.shape[0])
    loss = distance_consistency_loss(feats_t, feats_s, layers)

For sample i of a batch of B and its drawn layer l_i, the cosine similarities of sample i's whole feature map F_l[i] with the
feature maps of the other B - 1 samples at the same layer form a row; a softmax turns the row into a distribution; the loss is
the KL divergence of the adapted generator's distributions from the source's.  This docstring is the specification:

    c[i][k]   = cos(F_{l_i}[i], F_{l_i}[j]),   j != i ascending                                        [B, B - 1]
    cos(a, b) = <a, b> / (max(|a|, eps) max(|b|, eps)),   eps = 1e-8       (torch.nn.functional.cosine_similarity)
    p_s       = softmax(rows of the source's c)              (no gradient)
    log p_t   = log_softmax(rows of the target's c)
    loss      = mean over all B (B - 1) entries of p_s (log p_s - log p_t)         (nn.KLDivLoss(), reduction 'mean')

Every cosine of one layer comes from one Gram matrix G = X X^T of the B flattened feature maps (``gram``): one pass over the
features per DISTINCT drawn layer, instead of one pass per pair.  On the device ``gram`` runs rick_gram_f32 (fp32 products in
fixed-order FMA chains, slices added in fp64: G is bit-identical from run to run, exactly symmetric, and G[i][j] depends on rows
i and j alone) and its backward pass dX = (gG + gG^T) X runs rick_rowmix_f32.  The kernels treat a sample's features as an
unordered bag of values, so channels-last activations are read as they lie.  CPU tensors, and batches above 8, take a torch
composition that accumulates in fp64.  Everything after the Gram matrix is [B, B] fp64 tensor work.
"""
import numpy as np
import torch

EPS = 1e-8               # torch.nn.functional.cosine_similarity's default
MAX_B = 8                # rick_gram_f32 / rick_rowmix_f32


def _sample_dense(x):
    """True if every sample x[i] occupies one dense block of memory (in any dimension order) and the blocks follow each other
    at a stride of the block's size: the [B, n] row view the kernels read."""
    n = x[0].numel() if x.shape[0] else 0
    dims = sorted((st, sz) for st, sz in zip(x.stride()[1:], x.shape[1:]) if sz > 1)
    expect = 1
    for st, sz in dims:
        if st != expect:
            return False
        expect *= sz
    return x.shape[0] <= 1 or x.stride(0) == n


def _rows(x):
    """[B, n] view of a sample-dense x in memory order."""
    n = x[0].numel()
    return torch.as_strided(x, (x.shape[0], n), (n, 1), x.storage_offset())


def _use_kernels(x):
    return x.is_cuda and 1 <= x.shape[0] <= MAX_B


def _gram_rows(rows):
    """rick_gram_f32 on a [B, n] fp32 device tensor with row stride n -> [B, B] fp64."""
    from . import _lib
    B, n = rows.shape
    G = torch.empty((B, B), device=rows.device, dtype=torch.float64)
    with torch.cuda.device(rows.device):
        ws = torch.empty(_lib.lib.rick_gram_workspace_bytes(B, n) // 4, device=rows.device, dtype=torch.float32)
        _lib.check(_lib.lib.rick_gram_f32(rows.data_ptr(), B, n, ws.data_ptr(), G.data_ptr(), _lib.stream_ptr()), 'rick_gram_f32')
    return G


def rowmix(A, rows, out=None):
    """y[k] = sum_m A[k][m] rows[m] on rick_rowmix_f32: A [B, B] and rows [B, n] (row stride n) fp32 on the device, B <= 8; A
    is read from device memory (no host copy).  With A = I it returns rows bit for bit.  No autograd."""
    from . import _lib
    B, n = rows.shape
    if out is None:
        out = torch.empty_like(rows)
    for t in (A, rows, out):
        if not t.is_cuda or t.dtype != torch.float32 or t.device != rows.device:
            raise RuntimeError('cdc.rowmix: float32 tensors on one device')
    if tuple(A.shape) != (B, B) or out.shape != rows.shape or not 1 <= B <= MAX_B or n < 1:
        raise ValueError(f'cdc.rowmix: A {tuple(A.shape)}, rows {tuple(rows.shape)}, out {tuple(out.shape)}')
    if (B > 1 and (rows.stride(0) != n or out.stride(0) != n)) or (n > 1 and (rows.stride(1) != 1 or out.stride(1) != 1)):
        raise ValueError('cdc.rowmix: rows and out must have row stride n')
    A = A.contiguous()
    with torch.cuda.device(rows.device):
        _lib.check(_lib.lib.rick_rowmix_f32(A.data_ptr(), rows.data_ptr(), out.data_ptr(), B, n, _lib.stream_ptr()), 'rick_rowmix_f32')
    return out


class _Gram(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        xd = x.detach()
        if not _sample_dense(xd):
            xd = xd.contiguous()
        rows = _rows(xd)
        if _use_kernels(xd):
            G = _gram_rows(rows)
        else:
            r64 = rows.double()
            G = torch.triu(r64 @ r64.t())
            G = G + torch.triu(G, 1).t()                   # exactly symmetric, like the kernel's
        ctx.save_for_backward(xd)
        return G

    @staticmethod
    def backward(ctx, gG):
        if torch.is_grad_enabled():
            raise RuntimeError('cdc.gram: the backward pass is first order only (create_graph=True is not supported)')
        (xd,) = ctx.saved_tensors
        A = gG + gG.t()
        gx = torch.empty_like(xd)                          # dense like xd: the gradient in the layout of x
        rows = _rows(xd)
        if _use_kernels(xd):
            rowmix(A.to(torch.float32), rows, out=_rows(gx))
        else:
            _rows(gx).copy_(A.double() @ rows.double())
        return gx


def gram(x):
    """x [B, ...] fp32 -> G [B, B] fp64, G[i][j] = <x[i], x[j]> over all elements of a sample.  Differentiable with respect to
    x, first order only (``create_graph=True`` raises in the backward pass); the gradient has x's layout.  Each sample must be
    one dense block of memory in any dimension order (contiguous, channels-last, ...); anything else is copied first."""
    if x.dim() < 1 or x.shape[0] < 1 or x[0].numel() < 1:
        raise ValueError(f'cdc.gram: expected [B >= 1, ...] with at least one element per sample, got {tuple(x.shape)}')
    if x.dtype != torch.float32:
        raise RuntimeError(f'cdc.gram: features must be float32, got {x.dtype}')
    return _Gram.apply(x)


def pairwise_cosine(feats, layers):
    """feats: the generator's feature list (``Generator.forward(..., return_feats=True)``), each [B, ...] fp32; layers: B layer
    indices -> [B, B - 1] fp64, row i = cos(feats[l_i][i], feats[l_i][j]) for j != i ascending, from one ``gram`` per distinct
    layer.  The cosine is torch.nn.functional.cosine_similarity's with its default eps, applied to G_ij, G_ii, G_jj in fp64."""
    layers = [int(l) for l in layers]
    B = len(layers)
    if B < 2:
        raise ValueError('cdc.pairwise_cosine: needs at least two samples')
    rows = [None] * B
    for l in sorted(set(layers)):
        f = feats[l]
        if f.shape[0] != B:
            raise ValueError(f'cdc.pairwise_cosine: layer {l} holds {f.shape[0]} samples, layers has {B} entries')
        G = gram(f)
        norm = torch.diagonal(G).clamp_min(EPS * EPS).sqrt()               # max(|x|, eps), with a zero gradient below eps
        C = G / (norm[:, None] * norm[None, :])
        for i in range(B):
            if layers[i] == l:
                rows[i] = torch.cat([C[i, :i], C[i, i + 1:]])
    return torch.stack(rows)


def distance_consistency_loss(feats_target, feats_source, layers):
    """The loss of the module docstring: 0-dim fp32.  Gradients flow into feats_target only."""
    with torch.no_grad():
        log_ps = torch.log_softmax(pairwise_cosine(feats_source, layers), 1)
        ps = log_ps.exp()
    log_pt = torch.log_softmax(pairwise_cosine(feats_target, layers), 1)
    return (ps * (log_ps - log_pt)).mean().to(torch.float32)


def draw_layers(n_latent, batch, rng=None):
    """One feature layer per sample, the customary draw: ``randint(1, n_latent - 1, size=batch)`` from ``rng`` (a
    numpy RandomState) or numpy's global state.  At 256 px (n_latent 14) it gives layers 1 ... 12 of the 13 features."""
    return (rng if rng is not None else np.random).randint(1, n_latent - 1, size=batch)
