"""Evaluation-time sampling (BASELINE config 4).

The reference's ``Evaluator.compute_inception_score`` (gan_training/eval.py:31-46) draws
``n_sample_store`` latents at a time, runs ``g_ema([z])`` and moves every image to the host as
NumPy until ``n_sample_test`` images exist; FID is then computed by a third-party Inception
network (rick_amd.inception runs it on the device; its weights are a download and are supplied by
the user).  This module keeps the
sampling loop on the device: the same batches, images written into one preallocated tensor, no
host round trips.  A feature extractor can be plugged in through ``feature_fn`` (called per
batch on device tensors) so a metric never needs the images on the host either.  ``intra_lpips`` is the
reference's intra-cluster LPIPS (eval.py:83-190) on the device, over rick_amd.lpips.  ``InceptionScoreStats`` /
``inception_score`` are the reference's Inception Score (gan_training/metrics/inception_score.py) streamed on the
device over rick_amd.inception.InceptionV3Logits; ``Evaluator.compute_inception_score(iscore=True)`` reports it.
"""
import math
import os

import numpy as np
import torch


@torch.no_grad()
def sample_images(g_ema, n_sample_test, n_sample_store=25, latent=512, generator=None, feature_fn=None,
                  out=None, latents=None):
    """Generate ``n_sample_test`` images in batches of ``n_sample_store`` (gan_training/eval.py:34-41).

    latents: optional [n, latent] tensor of fixed z (parity runs); otherwise z ~ N(0, I) from `generator`
    (a torch.Generator) or the default device RNG.  Returns (images[n_sample_test, 3, S, S] on device,
    features or None)."""
    was_training = g_ema.training
    g_ema.eval()
    dev = next(g_ema.parameters()).device
    size = g_ema.size
    if out is None:
        out = torch.empty((n_sample_test, 3, size, size), device=dev, dtype=torch.float32)
    feats = []
    done = 0
    while done < n_sample_test:
        nb = n_sample_store
        if latents is not None:
            z = latents[done:done + nb].to(dev)
            if z.shape[0] == 0:
                raise RuntimeError('sample_images: not enough fixed latents')
        else:
            z = torch.randn(nb, latent, device=dev, generator=generator)
        img, _ = g_ema([z])
        take = min(img.shape[0], n_sample_test - done)
        out[done:done + take].copy_(img[:take])
        if feature_fn is not None:
            feats.append(feature_fn(img[:take]))
        done += take
    if was_training:
        g_ema.train()
    return out, (torch.cat(feats, 0) if feats else None)


class FeatureStats:
    """Streaming mean / covariance of feature vectors on the device (fp64 accumulators).

    Replaces ``calculate_activation_statistics`` (gan_training/metrics/fid_score.py:132-142), which
    gathers every activation on the host and calls ``np.mean`` / ``np.cov(rowvar=False)``: here each
    batch adds ``sum x`` and ``x^T x`` (one hipBLAS GEMM) and the statistics are finalised once —
    no [n_samples, dims] array ever exists, on either side of PCIe."""

    def __init__(self, dims, device):
        self.n = 0
        self.sum = torch.zeros(dims, device=device, dtype=torch.float64)
        self.outer = torch.zeros(dims, dims, device=device, dtype=torch.float64)

    @torch.no_grad()
    def update(self, feats):
        f = feats.reshape(feats.shape[0], -1).to(torch.float64)
        if f.shape[1] != self.sum.shape[0]:
            raise RuntimeError(f'FeatureStats: expected {self.sum.shape[0]} features, got {f.shape[1]}')
        self.sum += f.sum(0)
        self.outer += f.t() @ f
        self.n += f.shape[0]
        return self

    def finalize(self):
        """-> (mu[dims], sigma[dims, dims]) with np.cov's default normalisation (n - 1)."""
        if self.n < 2:
            raise RuntimeError('FeatureStats: need at least two samples')
        mu = self.sum / self.n
        sigma = (self.outer - self.n * torch.outer(mu, mu)) / (self.n - 1)
        return mu, sigma


@torch.no_grad()
def frechet_distance(mu1, sigma1, mu2, sigma2):
    """d^2 = |mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr sqrt(S1 S2)   (fid_score.py:94-129), on the device.

    The reference takes scipy's ``sqrtm`` of the non-symmetric product and keeps the real part of its
    trace.  S1 S2 is similar to the symmetric PSD matrix S1^(1/2) S2 S1^(1/2), so the same trace is the sum
    of the square roots of that matrix's eigenvalues: two symmetric eigen-decompositions in fp64, no
    host round trip, and no singular-product fallback is needed (negative round-off eigenvalues clamp to 0)."""
    mu1, mu2 = mu1.to(torch.float64), mu2.to(torch.float64)
    s1, s2 = sigma1.to(torch.float64), sigma2.to(torch.float64)
    if mu1.shape != mu2.shape or s1.shape != s2.shape:
        raise RuntimeError('frechet_distance: statistics have different shapes')
    w, u = torch.linalg.eigh((s1 + s1.t()) * 0.5)
    s1h = (u * w.clamp_min(0).sqrt()) @ u.t()
    m = s1h @ s2 @ s1h
    lam = torch.linalg.eigvalsh((m + m.t()) * 0.5)
    tr_covmean = lam.clamp_min(0).sqrt().sum()
    diff = mu1 - mu2
    return diff.dot(diff) + torch.trace(s1) + torch.trace(s2) - 2 * tr_covmean


@torch.no_grad()
def fid_from_generator(g_ema, real_stats, feature_fn, n_sample_test=5000, n_sample_store=25, latent=512,
                       generator=None, latents=None):
    """BASELINE config 4 end to end on the device: sample ``n_sample_test`` images in batches of
    ``n_sample_store`` (gan_training/eval.py:31-46), push each batch through ``feature_fn`` (the Inception
    pool3 plug point: weights are supplied by the user, they are a download in the reference), accumulate
    the statistics, and return the Frechet distance to ``real_stats = (mu, sigma)``."""
    dev = next(g_ema.parameters()).device
    stats = None
    was_training = g_ema.training
    g_ema.eval()
    done = 0
    while done < n_sample_test:
        if latents is not None:
            z = latents[done:done + n_sample_store].to(dev)
        else:
            z = torch.randn(n_sample_store, latent, device=dev, generator=generator)
        img, _ = g_ema([z])
        img = img[:n_sample_test - done]
        f = feature_fn(img)
        if stats is None:
            stats = FeatureStats(f.reshape(f.shape[0], -1).shape[1], dev)
        stats.update(f)
        done += img.shape[0]
    if was_training:
        g_ema.train()
    mu, sigma = stats.finalize()
    return frechet_distance(mu, sigma, real_stats[0].to(dev), real_stats[1].to(dev))


@torch.no_grad()
def kid_from_features(codes_g, codes_r, n_subsets=100, subset_size=1000, degree=3, gamma=None, coef0=1, rng=None):
    """Kernel Inception Distance on the device: the unbiased polynomial-kernel MMD^2 of ``n_subsets`` random subsets
    (gan_metrics/kid_score.py:255-290 with the evaluator's arguments, :391-393) -> (mean, std, mmds[n_subsets]).

    The reference forms three subset_size^2 kernel matrices per subset with sklearn on the host; here each subset is
    three fp64 GEMMs + elementwise powers on the device.  Subset indices are drawn exactly like the reference does
    (``np.random.choice(n, subset_size, replace=False)``, generator first, then real; pass ``rng`` = a
    ``np.random.RandomState`` to make a run reproducible) so a seeded run reproduces the reference's subsets."""
    import numpy as np
    choice = (rng or np.random).choice
    xg, xr = codes_g.to(torch.float64), codes_r.to(torch.float64)
    if xg.shape[1] != xr.shape[1]:
        raise RuntimeError('kid_from_features: feature dimensions differ')
    if subset_size > min(xg.shape[0], xr.shape[0]):
        raise RuntimeError('kid_from_features: subset_size exceeds the number of samples')
    gam = 1.0 / xg.shape[1] if gamma is None else gamma
    m = subset_size
    mmds = torch.empty(n_subsets, dtype=torch.float64, device=xg.device)
    for i in range(n_subsets):
        ig = torch.as_tensor(choice(xg.shape[0], subset_size, replace=False), device=xg.device)
        ir = torch.as_tensor(choice(xr.shape[0], subset_size, replace=False), device=xr.device)
        g, r = xg[ig], xr[ir]
        k_xx = (gam * (g @ g.t()) + coef0) ** degree
        k_yy = (gam * (r @ r.t()) + coef0) ** degree
        k_xy = (gam * (g @ r.t()) + coef0) ** degree
        kt_xx = k_xx.sum() - torch.diagonal(k_xx).sum()          # off-diagonal sums
        kt_yy = k_yy.sum() - torch.diagonal(k_yy).sum()
        mmds[i] = (kt_xx + kt_yy) / (m * (m - 1)) - 2 * k_xy.sum() / (m * m)
    return mmds.mean(), mmds.std(unbiased=False), mmds


def clip_similarity(fa, fb):
    """Cosine similarities of two sets of embeddings, fa [na, D] and fb [nb, D] -> [na, nb] in fp64 on fa's device: the quantity
    image-guided StyleGAN-NADA and "similarity to the few-shot targets" both start from (rick_amd/clip.py returns the
    unnormalised embeddings)."""
    if fa.dim() != 2 or fb.dim() != 2 or fa.shape[1] != fb.shape[1]:
        raise RuntimeError(f'clip_similarity: expected [na, D] and [nb, D], got {tuple(fa.shape)} and {tuple(fb.shape)}')
    a, b = fa.double(), fb.double().to(fa.device)
    return (a / a.norm(dim=1, keepdim=True)) @ (b / b.norm(dim=1, keepdim=True)).T


@torch.no_grad()
def precision_recall_from_features(feats_real, feats_fake, k=3, block=4096):
    """Improved precision / recall (gan_metrics/precision_recall.py:50-66, 185-246) on the device.

    Each set defines a manifold = union of balls around its features with radius = distance to the k-th nearest
    neighbour in the same set; precision = share of fake features inside the real manifold, recall = share of real
    features inside the fake one.  The reference builds the N x N distance matrices with NumPy on the host and loops
    over rows; here they are fp64 GEMM blocks on the device (`block` columns at a time) reduced with kthvalue / any.
    Returns (precision, recall) as 0-dim device tensors."""
    xr, xf = feats_real.to(torch.float64), feats_fake.to(torch.float64)
    if xr.shape[1] != xf.shape[1]:
        raise RuntimeError('precision_recall_from_features: feature dimensions differ')
    if min(xr.shape[0], xf.shape[0]) <= k:
        raise RuntimeError('precision_recall_from_features: need more than k samples per set')

    def dist(a, b):                       # [len(a), len(b)] Euclidean distances, negative round-off clamped like the reference
        d2 = (a * a).sum(1, keepdim=True) - 2 * (a @ b.t()) + (b * b).sum(1).unsqueeze(0)
        return d2.clamp_min(0).sqrt()

    def radii(x):                         # k-th neighbour = (k+1)-th smallest of the row (the closest one is the point itself)
        out = torch.empty(x.shape[0], dtype=torch.float64, device=x.device)
        for lo in range(0, x.shape[0], block):
            out[lo:lo + block] = dist(x[lo:lo + block], x).kthvalue(k + 1, dim=1).values
        return out

    def covered(ref, ref_radii, subj):    # share of subjects inside at least one ball of the reference manifold
        hit = 0
        for lo in range(0, subj.shape[0], block):
            hit = hit + (dist(ref, subj[lo:lo + block]) < ref_radii.unsqueeze(1)).any(0).sum()
        return hit.to(torch.float64) / subj.shape[0]
    return covered(xr, radii(xr), xf), covered(xf, radii(xf), xr)


class InceptionScoreStats:
    """The Inception Score (gan_training/metrics/inception_score.py:12-58) streamed on the device.

    The reference stores softmax(logits) of all N images in a float64 [N, 1000] host array, cuts it into ``splits`` runs of
    ``per = N // splits`` rows (the rest is dropped) and returns the mean and population std over the splits of
    exp(mean_i KL(p_i || py)), with scipy.stats.entropy renormalising both arguments.  Here every batch is reduced at once
    to a state [splits, 2 C + 1] fp64: per split the class sums P of p, the class sums Q of q_i = p_i / sum_c p_ic and
    H = sum_i sum_c q_ic log q_ic.  With n = per, py = P / n and qy = py / sum py the split's score is
    exp(H / n - sum_c (Q_c / n) log qy_c), the same quantity.  On the device the rows come from rick_is_rows_f32 and are
    folded by rick_is_accum_f64, which adds rows in ascending order: the state does not depend on how the sample was cut
    into batches.  CPU tensors take the same steps in torch.

    net: images -> logits [N, C] (``rick_amd.inception.InceptionV3Logits``); n_total: the N of the reference's call."""

    def __init__(self, net, n_total, splits=1):
        if splits < 1:
            raise ValueError(f'InceptionScoreStats: splits must be >= 1, got {splits}')
        if n_total // splits < 1:
            raise ValueError(f'InceptionScoreStats: {n_total} samples cannot fill {splits} splits')
        self.net, self.n_total, self.splits, self.per = net, int(n_total), int(splits), int(n_total) // int(splits)
        self.seen, self.acc = 0, None

    @torch.no_grad()
    def update_logits(self, logits):
        """Fold logits [M, C] fp32, the next M rows of the sample."""
        if logits.dim() != 2 or logits.dtype != torch.float32:
            raise RuntimeError(f'InceptionScoreStats: expected fp32 logits [M, C], got {logits.dtype} {tuple(logits.shape)}')
        M, C = logits.shape
        if self.acc is None:
            self.acc = torch.zeros((self.splits, 2 * C + 1), device=logits.device, dtype=torch.float64)
        if self.acc.shape[1] != 2 * C + 1 or self.acc.device != logits.device:
            raise RuntimeError(f'InceptionScoreStats: the state is {tuple(self.acc.shape)} on {self.acc.device}, got logits '
                               f'{tuple(logits.shape)} on {logits.device}')
        if logits.device.type == 'cpu':
            p = torch.softmax(logits, dim=-1)
            s = p.double().sum(1)
            q = p.double() / s[:, None]
            h = torch.xlogy(q, q).sum(1)
            for i in range(M):                                  # ascending rows, one at a time: the kernel's order
                g = self.seen + i
                if g < self.splits * self.per:
                    k = g // self.per
                    self.acc[k, :C] += p[i].double()
                    self.acc[k, C:2 * C] += q[i]
                    self.acc[k, 2 * C] += h[i]
        else:
            from .inception import accumulate_rows, softmax_rows
            p, s, h = softmax_rows(logits)
            accumulate_rows(self.acc, p, s, h, self.seen, self.per)
        self.seen += M
        return self

    @torch.no_grad()
    def update(self, images):
        """Push a batch of images through the network and fold its rows; nothing leaves the device."""
        return self.update_logits(self.net(images))

    @torch.no_grad()
    def finalize(self):
        """-> (mean, std) over the splits as fp64 0-dim tensors on the state's device (std: population, 0 for one split)."""
        if self.acc is None or self.seen < self.splits * self.per:
            raise RuntimeError(f'InceptionScoreStats: {self.seen} of {self.splits * self.per} samples seen')
        C, n = (self.acc.shape[1] - 1) // 2, float(self.per)
        P, Q, H = self.acc[:, :C], self.acc[:, C:2 * C], self.acc[:, 2 * C]
        py = P / n
        qy = py / py.sum(1, keepdim=True)
        scores = torch.exp(H / n - torch.xlogy(Q / n, qy).sum(1))
        return scores.mean(), scores.std(unbiased=False)


@torch.no_grad()
def inception_score(images, net, splits=1):
    """The reference's ``inception_score(imgs, resize=..., splits=...)`` on an image tensor [N, 3, H, W] -> (mean, std);
    whether the images are resized is a property of ``net`` (``InceptionV3Logits.load(size=...)``)."""
    stats = InceptionScoreStats(net, images.shape[0], splits)
    step = int(getattr(net, 'batch', 100))
    for lo in range(0, images.shape[0], step):
        stats.update(images[lo:lo + step])
    return stats.finalize()


def lpips_sample_count(n_samples=1000, n_sample_store=25, fid_sample_size=5000):
    """Images the reference's compute_intra_lpips keeps (eval.py:86-92): whole batches of ``n_sample_store`` until at
    least ``n_samples`` exist, then the first ``fid_sample_size``."""
    return min(-(-n_samples // n_sample_store) * n_sample_store, fid_sample_size)


def assign_clusters(dist):
    """dist [n, K] (sample-to-centre LPIPS) -> [n] int64: the nearest centre, ties to the lowest index (np.argmin)."""
    return torch.from_numpy(np.argmin(np.asarray(torch.as_tensor(dist).cpu(), dtype=np.float64), axis=1).astype(np.int64))


def cluster_subsets(assign, k, cluster_size=50, rng=None):
    """Members of each of the k clusters in sample order; a cluster with more than ``cluster_size`` members keeps
    ``members[torch.randperm(count, generator=rng)[:cluster_size]]``.  The reference shuffles a directory listing with
    ``random.shuffle`` (eval.py:170-171), which no seed reproduces; a torch.Generator makes the draw reproducible."""
    assign = torch.as_tensor(assign).cpu()
    out = []
    for c in range(k):
        idx = torch.nonzero(assign == c).flatten()
        if idx.numel() > cluster_size:
            idx = idx[torch.randperm(idx.numel(), generator=rng)[:cluster_size]]
        out.append(idx)
    return out


def mean_pair_distance(d):
    """Mean of d[i, j] over the unordered pairs i < j of a square distance matrix (fp64); NaN below two members."""
    d = torch.as_tensor(d).to('cpu', torch.float64)
    m = d.shape[0]
    if m < 2:
        return math.nan
    iu = torch.triu_indices(m, m, 1)
    return float(d[iu[0], iu[1]].mean())


def nan_mean(values):
    """Mean of the non-NaN values (eval.py:189); NaN if there are none."""
    v = torch.as_tensor(values, dtype=torch.float64)
    v = v[~torch.isnan(v)]
    return float(v.mean()) if v.numel() else math.nan


@torch.no_grad()
def intra_lpips(g_ema, centers, lpips, n_samples=1000, n_sample_store=25, cluster_size=50, fid_sample_size=5000, latent=512,
                size=256, latents=None, rng=None):
    """Intra-cluster LPIPS (gan_training/eval.py:83-190) on the device -> (value, per_cluster [K] fp64 with NaN, counts [K]).

    centers: uint8 [K, 3, size, size] (``load_cluster_centers``); lpips: a ``rick_amd.lpips.LPIPS``.  The samples go through
    the reference's PNG round trip (uint8, read back as q / 255) and stay on the device as uint8.  Pass 1: each batch's
    LPIPS features, its distances to the K centres (whose features are computed once), then the nearest centre of every
    sample.  Pass 2: per cluster, at most ``cluster_size`` members (``cluster_subsets``, drawn from ``rng``), their features
    recomputed from the stored uint8 images (bit-identical to pass 1's: the trunk is batch-invariant) and the mean LPIPS over
    all their unordered pairs.  ``value`` is the mean over the clusters with at least two members (NaN if none).  Images
    whose size is not ``size`` are refused, as the reference's Resize([256, 256]) is the identity only there."""
    dev = next(g_ema.parameters()).device
    if centers.dim() != 4 or centers.shape[1] != 3 or tuple(centers.shape[2:]) != (size, size):
        raise ValueError(f'intra_lpips: centres must be [K, 3, {size}, {size}], got {tuple(centers.shape)}')
    if centers.dtype != torch.uint8:
        raise ValueError(f'intra_lpips: centres must be uint8 (the PNG files), got {centers.dtype}')
    n = lpips_sample_count(n_samples, n_sample_store, fid_sample_size)
    K = centers.shape[0]
    fc = lpips.features(centers.to(dev).contiguous())
    store = torch.empty((n, 3, size, size), device=dev, dtype=torch.uint8)
    dist = torch.empty((n, K), device=dev, dtype=torch.float32)
    ws = lpips.workspace_features if dev.type == 'cuda' and n_sample_store <= lpips.batch and lpips.size == size else None
    was_training = g_ema.training
    g_ema.eval()
    done = 0
    while done < n:
        if latents is not None:
            z = latents[done:done + n_sample_store].to(dev)
            if z.shape[0] == 0:
                raise RuntimeError('intra_lpips: not enough fixed latents')
        else:
            z = torch.randn(n_sample_store, latent, device=dev)
        img, _ = g_ema([z])
        if tuple(img.shape[2:]) != (size, size):
            raise ValueError(f'intra_lpips: generated images are {tuple(img.shape[2:])}, the evaluation size is {size}')
        take = min(img.shape[0], n - done)
        f = lpips.features(img[:take].contiguous(), quantize=True, out=ws, u8_out=store[done:done + take])
        dist[done:done + take] = lpips.distances(f, fc)
        done += take
    if was_training:
        g_ema.train()
    assign = assign_clusters(dist)
    counts = torch.bincount(assign, minlength=K)
    per = torch.full((K,), math.nan, dtype=torch.float64)
    subsets = cluster_subsets(assign, K, cluster_size, rng)
    fs = None
    for c, idx in enumerate(subsets):
        if idx.numel() < 2:
            continue
        if fs is None and dev.type == 'cuda':
            fs = lpips.new_features(max(s.numel() for s in subsets), size, size)
        f = lpips.features(store[idx.to(dev)], out=fs)
        per[c] = mean_pair_distance(lpips.distances(f, f))
    return nan_mean(per), per, counts


def load_cluster_centers(root, k=10):
    """The reference's cluster centres (``../cluster_centers/<data>/<method>/c{i}/center.png``, eval.py:122-124) -> uint8
    [k, 3, S, S], decoded with rick_amd.data.decode_png."""
    from .data import decode_png
    imgs = []
    for i in range(k):
        with open(os.path.join(root, f'c{i}', 'center.png'), 'rb') as fh:
            imgs.append(decode_png(fh.read()))
    if len({im.shape for im in imgs}) != 1:
        raise ValueError(f'load_cluster_centers: centres of different sizes {sorted({im.shape for im in imgs})}')
    return torch.from_numpy(np.stack(imgs)).permute(0, 3, 1, 2).contiguous()


class Evaluator:
    """Device-resident counterpart of ``gan_training.eval.Evaluator`` (eval.py:13-66).

    The reference keeps the real images in ``real_imgs.npy``, generates ``inception_nsamples`` fakes onto the host and
    hands both image sets to three separate metric modules, each of which runs its own Inception / VGG forward pass.
    Here the real side is reduced ONCE to features (``real_feats [n, dims]``, any device tensor), every generated batch
    goes through ``feature_fn`` while it is still on the GPU, and FID / KID / precision-recall are all computed from the
    same two feature matrices.  ``feature_fn`` is the plug point for the pretrained networks (weights are downloads in
    the reference; the reference uses Inception pool3 for FID / KID and VGG-16 fc2 for precision-recall — pass
    ``pr_feature_fn`` / ``real_pr_feats`` to keep that split)."""

    def __init__(self, generator, feature_fn, real_feats, n_sample_store=25, latent=512, inception_nsamples=5000,
                 fid_sample_size=5000, pr_feature_fn=None, real_pr_feats=None, k=3, is_net=None):
        self.is_net = is_net
        self.generator, self.feature_fn, self.real_feats = generator, feature_fn, real_feats
        self.n_sample_store, self.latent = n_sample_store, latent
        self.inception_nsamples, self.sample_size, self.k = inception_nsamples, fid_sample_size, k
        self.pr_feature_fn, self.real_pr_feats = pr_feature_fn, real_pr_feats

    @torch.no_grad()
    def compute_inception_score(self, fid=True, kid=False, pr=False, latents=None, kid_subsets=100, kid_subset_size=1000,
                                rng=None, iscore=False, is_splits=1):
        """-> dict with 'fid', 'kid', 'precision', 'recall' (the keys the reference fills, eval.py:44-66); iscore=True adds
        'is' and 'is_std', the Inception Score of the first ``fid_sample_size`` generated images over ``is_splits`` splits
        (``is_net``: a ``rick_amd.inception.InceptionV3Logits``), streamed batch by batch through InceptionScoreStats."""
        g = self.generator
        dev = next(g.parameters()).device
        is_stats = None
        if iscore:
            if self.is_net is None:
                raise RuntimeError('Evaluator: iscore=True needs is_net')
            n_gen = -(-self.inception_nsamples // self.n_sample_store) * self.n_sample_store
            if latents is not None:
                n_gen = min(n_gen, latents.shape[0])
            is_stats = InceptionScoreStats(self.is_net, min(n_gen, self.sample_size), is_splits)
        was_training = g.training
        g.eval()
        feats, pr_feats, done = [], [], 0
        while done < self.inception_nsamples:                       # eval.py:34-41: batches of n_sample_store
            if latents is not None:
                z = latents[done:done + self.n_sample_store].to(dev)
            else:
                z = torch.randn(self.n_sample_store, self.latent, device=dev)
            img, _ = g([z])
            feats.append(self.feature_fn(img).reshape(img.shape[0], -1))
            if pr and self.pr_feature_fn is not None:
                pr_feats.append(self.pr_feature_fn(img).reshape(img.shape[0], -1))
            if is_stats is not None and done < is_stats.n_total:
                is_stats.update(img[:is_stats.n_total - done])
            done += img.shape[0]
        if was_training:
            g.train()
        fake = torch.cat(feats, 0)[:self.sample_size]
        real = self.real_feats.to(dev)
        score = {}
        if fid:
            st_r, st_f = FeatureStats(real.shape[1], dev).update(real), FeatureStats(fake.shape[1], dev).update(fake)
            score['fid'] = frechet_distance(*st_r.finalize(), *st_f.finalize())
        if kid:                                                     # eval.py:52-54: the first 2000 of each side
            score['kid'] = kid_from_features(real[:2000], fake[:2000], n_subsets=kid_subsets, subset_size=kid_subset_size,
                                             rng=rng)[0]
        if pr:
            fr = self.real_pr_feats.to(dev) if self.real_pr_feats is not None else real
            ff = torch.cat(pr_feats, 0)[:self.sample_size] if pr_feats else fake
            score['precision'], score['recall'] = precision_recall_from_features(fr, ff, k=self.k)
        if is_stats is not None:
            score['is'], score['is_std'] = is_stats.finalize()
        return score

    def compute_intra_lpips(self, centers, lpips, n_samples=1000, cluster_size=50, size=256, latents=None, rng=None):
        """The reference's ``compute_intra_lpips(args)`` (eval.py:83-107) -> the intra-cluster LPIPS (see ``intra_lpips``)."""
        return intra_lpips(self.generator, centers, lpips, n_samples=n_samples, n_sample_store=self.n_sample_store,
                           cluster_size=cluster_size, fid_sample_size=self.sample_size, latent=self.latent, size=size,
                           latents=latents, rng=rng)[0]

    def compute_ppl(self, lpips, **kw):
        """The perceptual path length of the generator (``rick_amd.ppl.perceptual_path_length``, whose keywords ``kw`` are)
        -> the filtered mean."""
        from .ppl import perceptual_path_length
        return perceptual_path_length(self.generator, lpips, **kw)[0]
