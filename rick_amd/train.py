"""Host side of the RICK adaptation loop on the MI355X engine: losses and gradient penalties,
the Fisher-information sweep with on-device grad^2 accumulation and per-filter reduction, the
freeze / fine-tune / prune decisions and masks (flat masked Adam + EMA: rick_amd/flat.py), and the per-iteration
control flow of ``train()`` (train_dynamic_update_prune.py:159-699).

Work the reference performs and then discards is skipped (SURVEY.md §8a footnote): the D step
runs on ``fake.detach()``, the G step does not compute D weight gradients, and parameters that
no optimiser owns do not get gradients.  Results are unchanged.
"""
import math
import os
import random
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F
from torch import autograd

from . import op
from ._lib import check, lib, ptr, stream_ptr
from . import augment as A
from . import diffaug as DA
from . import gterms
from .augment import augment_fused
from .diffaug import diffaug_fused
from .flat import FLAT_ALIGN, FisherAccumulator, FlatParams, MaskedFlatAdam, ema_flat  # noqa: F401  (re-exported)
from .param_block import StepParamBlock


# --------------------------------------------------------------------------- losses
def d_logistic_loss(real_pred, fake_pred):
    """train_dynamic_update_prune.py:82-86"""
    return F.softplus(-real_pred).mean() + F.softplus(fake_pred).mean()


def g_nonsaturating_loss(fake_pred):
    """train_dynamic_update_prune.py:99-101"""
    return F.softplus(-fake_pred).mean()


def d_r1_loss(real_pred, real_img):
    """train_dynamic_update_prune.py:89-96 (needs op.second_order())."""
    with op.no_param_grads():      # the inner gradient is w.r.t. the image only: no weight-gradient launches for it
        (grad_real,) = autograd.grad(outputs=real_pred.sum(), inputs=real_img, create_graph=True)
    return grad_real.pow(2).reshape(grad_real.shape[0], -1).sum(1).mean()


def g_path_regularize(fake_img, latents, mean_path_length, decay=0.01, noise=None):
    """train_dynamic_update_prune.py:104-118 (needs op.second_order()).  `noise` overrides the
    randn_like draw so parity tests can share it with the oracle."""
    if noise is None:
        noise = torch.randn_like(fake_img)
    noise = noise / math.sqrt(fake_img.shape[2] * fake_img.shape[3])
    with op.no_param_grads():      # the inner gradient is w.r.t. the latents only
        (grad,) = autograd.grad(outputs=(fake_img * noise).sum(), inputs=latents, create_graph=True)
    path_lengths = torch.sqrt(grad.pow(2).sum(2).mean(1))
    path_mean = mean_path_length + decay * (path_lengths.mean() - mean_path_length)
    path_penalty = (path_lengths - path_mean).pow(2).mean()
    return path_penalty, path_mean.detach(), path_lengths


def make_noise(batch, latent_dim, n_noise, device):
    if n_noise == 1:
        return torch.randn(batch, latent_dim, device=device)
    return torch.randn(n_noise, batch, latent_dim, device=device).unbind(0)


def mixing_noise(batch, latent_dim, prob, device):
    """train_dynamic_update_prune.py:130-135"""
    if prob > 0 and random.random() < prob:
        return make_noise(batch, latent_dim, 2, device)
    return [make_noise(batch, latent_dim, 1, device)]


def requires_grad(model, flag=True, only=None):
    for name, p in model.named_parameters():
        if only is None or only(name):
            p.requires_grad = flag


# ------------------------------------------------------------------------ Fisher sweep
def filter_mean(t, filter_dim):
    """Mean over every dim except `filter_dim` with one wavefront per filter
    (rick_filter_reduce_f32).  Supports filter_dim 0 ([F, ...]) and 1 of a [1, F, ...] tensor."""
    t = t.contiguous()
    if filter_dim == 1:
        if t.shape[0] != 1:
            raise RuntimeError('filter_mean: dim-1 filters need a leading dim of 1')
        t = t[0]
    nf = t.shape[0]
    inner = t.numel() // nf
    out = torch.empty(nf, device=t.device, dtype=t.dtype)
    check(lib.rick_filter_reduce_f32(ptr(t), ptr(out), 1, 0, nf, inner, inner, 1.0 / inner, stream_ptr()),
          'rick_filter_reduce_f32')
    return out


def g_filter_fim(fisher, n_blocks=None):
    """Per-filter FIM of the generator (train_dynamic_update_prune.py:279-299): dicts of device vectors."""
    conv, fc = {}, {}
    if n_blocks is None:      # 12 at 256 px, the only size the reference supports (hard-coded range(12), :281)
        n_blocks = sum(1 for k in fisher if k.startswith('convs.') and k.endswith('.conv.weight'))
    for k in range(n_blocks):
        conv[f'convs.{k}.conv.weight'] = filter_mean(fisher[f'convs.{k}.conv.weight'], 1)
        wk = f'convs.{k}.conv.modulation.weight'
        fc[wk] = (filter_mean(fisher[wk], 0) + fisher[f'convs.{k}.conv.modulation.bias']) / 2
    return conv, fc


def d_filter_fim(fisher, blocks=None):
    """Per-filter FIM of the discriminator (train_dynamic_update_prune.py:334-353)."""
    out = {}
    if blocks is None:        # range(1, 7) at 256 px (:336)
        blocks = range(1, 1 + sum(1 for k in fisher if k.endswith('.skip.1.weight')))
    for b in blocks:
        for li in range(2):
            wk, bk = f'convs.{b}.conv{li + 1}.{li}.weight', f'convs.{b}.conv{li + 1}.{li + 1}.bias'
            out[wk] = (filter_mean(fisher[wk], 0) + fisher[bk]) / 2
            if li == 1:
                sk = f'convs.{b}.skip.{li}.weight'
                out[sk] = filter_mean(fisher[sk], 0)
    return out


def _split(fim, cut, prune, skip_rule=False):
    if skip_rule:   # train_dynamic_update_prune.py:382-384
        return np.where(fim > cut)[0], np.where((fim >= prune) & (fim <= cut))[0], np.where(fim < prune)[0]
    return np.where(fim > cut)[0], np.where((fim > prune) & (fim <= cut))[0], np.where(fim <= prune)[0]


def decide_g(conv, fc, fisher_quantile, prune_quantile):
    """freeze / ft / prune index sets of the generator from per-filter FIM vectors (host numpy,
    a few thousand floats; np.percentile in PERCENT units — train_dynamic_update_prune.py:285-330)."""
    conv = {k: np.asarray(v, dtype=np.float32) for k, v in conv.items()}
    fc = {k: np.asarray(v, dtype=np.float32) for k, v in fc.items()}
    allc = np.concatenate([[]] + list(conv.values()), axis=None)
    allf = np.concatenate([[]] + list(fc.values()), axis=None)
    cut_c, pr_c = np.percentile(allc, q=fisher_quantile), np.percentile(allc, q=prune_quantile)
    cut_f, pr_f = np.percentile(allf, q=fisher_quantile), np.percentile(allf, q=prune_quantile)
    freeze, ft, prune = {}, {}, {}
    for k, v in conv.items():
        freeze[k], ft[k], prune[k] = _split(v, cut_c, pr_c)
    for k, v in fc.items():
        for kk in (k, k.replace('weight', 'bias')):
            freeze[kk], ft[kk], prune[kk] = _split(v, cut_f, pr_f)
    return freeze, ft, prune


def decide_d(fim, fisher_quantile, prune_quantile):
    """train_dynamic_update_prune.py:352-384"""
    fim = {k: np.asarray(v, dtype=np.float32) for k, v in fim.items()}
    allv = np.concatenate([[]] + list(fim.values()), axis=None)
    cut, pr = np.percentile(allv, q=fisher_quantile), np.percentile(allv, q=prune_quantile)
    freeze, ft, prune = {}, {}, {}
    for k, v in fim.items():
        if 'skip' in k:
            freeze[k], ft[k], prune[k] = _split(v, cut, pr, skip_rule=True)
        else:
            bk = k.replace(f'{k[-8]}.weight', f'{int(k[-8]) + 1}.bias')
            for kk in (k, bk):
                freeze[kk], ft[kk], prune[kk] = _split(v, cut, pr)
    return freeze, ft, prune


def zero_idx_merge(old, new):
    """train_dynamic_update_prune.py:138-144"""
    return {k: np.unique(np.concatenate((old[k], new[k]))) for k in old}


def build_mask(flat, freeze_idx, zero_idx):
    """Flat uint8 mask for MaskedFlatAdam from per-key filter index sets: bit0 = freeze
    (grad := 0), bit1 = zero/prune (param := 0, grad := 0).  5-D generator conv weights are
    indexed on dim 1, everything else on dim 0 (train_dynamic_update_prune.py:524-537, 429-435)."""
    mask = np.zeros(flat.total, dtype=np.uint8)      # plain NumPy on the host: a few thousand contiguous filter rows
    for bit, table in ((1, freeze_idx), (2, zero_idx)):
        for name, idx in table.items():
            if name not in flat.index or len(idx) == 0:
                continue
            lo, hi = flat.segment(name)
            p = flat.params[flat.index[name]]
            view = mask[lo:hi].reshape(tuple(p.shape))
            ii = np.asarray(idx, dtype=np.int64)
            if p.ndim == 5:
                view[:, ii] |= bit
            else:
                view[ii] |= bit
    return torch.from_numpy(mask).to(flat.flat.device)


# --------------------------------------------------------------------------- trainer
@dataclass
class TrainConfig:
    """The live flags of the reference CLI (train_dynamic_update_prune.py:703-758) with its defaults."""
    size: int = 256
    batch: int = 4
    latent: int = 512
    n_mlp: int = 8
    channel_multiplier: int = 2
    r1: float = 10.0
    path_regularize: float = 2.0
    path_batch_shrink: int = 2
    d_reg_every: int = 16
    g_reg_every: int = 4
    mixing: float = 0.9
    lr: float = 0.002
    num_fisher_img: int = 5
    fisher_freq: int = 50
    fisher_quantile: float = 40.0
    prune_quantile: float = 0.1
    warmup_iter: int = 250
    ema_decay: float = 0.5 ** (32 / (10 * 1000))     # train_dynamic_update_prune.py:180
    augment: bool = False                            # adaptive discriminator augmentation (:728-732)
    augment_p: float = 0.0                           # > 0: fixed p; 0: p adapted from the sign of D's real logits
    ada_target: float = 0.6
    ada_length: int = 500 * 1000
    cdc_weight: float = 0.0                          # cross-domain distance consistency (rick_amd/cdc.py): the customary kl_wt, 1000
    cdc_batch: int = 4                               # its batch (the reference still parses it: --feat_const_batch, :707)
    ewc_weight: float = 0.0                          # elastic weight consolidation on the generator (rick_amd/ewc.py): the paper's 5e8
    kml_rank: int = 0                                # kernel modulation of the frozen filters (rick_amd/kml.py): AdAM's rank, 1 ... 8
    diffaug: str = ''                                # DiffAugment policy (rick_amd/diffaug.py), e.g. 'color,translation,cutout'; '' = off
    dcl_g_weight: float = 0.0                        # DCL's generator contrastive term CL1 (rick_amd/dcl.py): lambda1, recalled as 2 (unverified)
    dcl_d_weight: float = 0.0                        # DCL's discriminator contrastive term CL2: lambda2, recalled as 0.5 (unverified)
    dcl_tau: float = 0.07                            # the temperature of both terms
    dcl_batch: int = 4                               # CL1's own latent batch (like cdc_batch)
    svd_adapt: bool = False                          # FSGAN's singular-value adaptation of both networks (rick_amd/svd.py)
    svd_train_rest: bool = False                     # with svd_adapt: leave the non-adapted tensors (biases, ...) to the networks' Adam
    subspace_freq: int = 0                           # CDC's patch discriminator + anchor sampling (rick_amd/patchd.py): every subspace_freq-th iteration is an anchor iteration, the others patch-level; 0 = off (the reference's --subspace_freq defaults to 4, :708)
    subspace_std: float = 0.05                       # --subspace_std (:721)
    feat_ind: int = 3                                # --feat_ind (:709): p_ind is drawn from the first feat_ind taps
    n_anchors: int = 10                              # rows of the anchor matrix drawn at construction
    clip_dir_weight: float = 0.0                     # StyleGAN-NADA's directional loss in CLIP space (rick_amd/clipguide.py); 0 = off
    clip_within_weight: float = 0.0                  # Mind-the-Gap's in-domain consistency loss in CLIP space; 0 = off
    clip_batch: int = 4                              # the CLIP terms' own latent batch (like cdc_batch)


class AdaController:
    """The adaptive augmentation probability of the reference (train_dynamic_update_prune.py:440-459): signs of D's real logits
    are summed over steps; once more than 255 images are in, p moves by sign(mean - target) * ada_target / ada_length * n,
    clamped to [0, 1], and the sums restart.  With augment_p > 0, p stays fixed.

    The trainer keeps the sign sum on the device (no sync per step); the image count n is known on the host, so the device
    value is read (and, under data parallelism, summed over ranks) only when n > 255."""

    def __init__(self, cfg):
        self.adaptive = cfg.augment_p == 0
        self.p = float(cfg.augment_p) if cfg.augment_p > 0 else 0.0
        self.step_size = cfg.ada_target / cfg.ada_length
        self.target = cfg.ada_target
        self.n = 0

    def due(self, n_new):
        """Count n_new more images; True when the sign sum must be read (n > 255)."""
        if not self.adaptive:
            return False
        self.n += n_new
        return self.n > 255

    def update(self, sign_sum, n=None):
        """Apply the accumulated statistic (sign_sum over self.n images, or over `n` when given); returns the new p."""
        n = self.n if n is None else n
        sign = 1 if sign_sum / n > self.target else -1
        self.p = min(1.0, max(0.0, self.p + sign * self.step_size * n))
        self.n = 0
        return self.p


class StepAugmenter:
    """The discriminator-side augmentation of a trainer, ADA or DiffAugment (alternatives).  The recipes differ in two things:
    `draw(batch)`, the host records of one reference call, and `apply(x, dev)`, the fused op on a device parameter block.  Shared:
    `blocks`, the persistent parameter block of each step ('d', 'r1', 'g'; captured graphs read it), and `prepare`, the host side
    of a step's augmentation that its `pre=` hook calls."""

    def __init__(self, trainer):
        self.tr, self.blocks = trainer, {}

    def prepare(self, key, n_calls, batch, reverse=False):
        """One draw per reference call, in the reference's order, uploaded into the step's block (created on the first, eager
        call).  `n_calls` calls of `batch` images each; `reverse`: the launch's images are in the opposite order of the draws."""
        blk = self.blocks.get(key)
        if blk is None:
            blk = self.blocks[key] = StepParamBlock(self.itemsize, n_calls * batch, self.tr.device, self.who)
        return blk.fill([self.draw(batch) for _ in range(n_calls)], reverse)


class AdaAugmenter(StepAugmenter):
    """One (G, C) draw per call at the trainer's current p, or the trainer's `aug_source(n)` in the sampler's place."""
    itemsize, who = A.PARAM_DTYPE.itemsize, 'augment'

    def draw(self, batch):
        tr, size = self.tr, self.tr.cfg.size
        if tr.aug_source is not None:
            G, C = tr.aug_source(batch)
            G, pads = A.draw_affine(tr.ada.p, batch, size, size, G)
        else:
            G, pads = A.draw_affine(tr.ada.p, batch, size, size)
            C = A.sample_color(tr.ada.p, batch)
        return A.aug_params(G, C, size, size, pads)

    def apply(self, x, dev):
        return augment_fused(x, dev)


class DiffAugmenter(StepAugmenter):
    """The published trainer's draws of one call for the parsed policy, or the trainer's `diffaug_source(n)`, checked."""
    itemsize, who = DA.PARAM_DTYPE.itemsize, 'diffaug'

    def __init__(self, trainer, policy):
        super().__init__(trainer)
        self.policy = DA.parse_policy(policy)

    def draw(self, batch):
        tr, size = self.tr, self.tr.cfg.size
        rec = tr.diffaug_source(batch) if tr.diffaug_source is not None else DA.draw_params(batch, size, size, self.policy)
        return DA.check_params(rec, size, size)

    def apply(self, x, dev):
        return diffaug_fused(x, dev)


def g_optim_filter(name):
    return 'convs' in name                              # train_dynamic_update_prune.py:909-911


def d_optim_filter(name):
    return ('convs' in name and 'convs.0' not in name) or 'final' in name   # :922-926


class RickTrainer:
    """One process / one GPU worth of the adaptation loop.  `dp` (rick_amd.dist.DataParallelGrads
    or None) averages flat gradients over ranks with RCCL before each optimiser step.  The G step's extra loss terms are
    rick_amd/gterms.py's (`g_terms`: the ones switched on; each checks its own configuration and resources).  `g_source`: the
    frozen source generator those terms and the discriminator contrastive term need (put in eval mode, gradients off);
    `d_source`: the frozen source discriminator of the discriminator contrastive term (required with g_source when
    cfg.dcl_d_weight > 0; treated like g_source).  `ewc`: the
    anchor of the elastic-weight-consolidation term (required when cfg.ewc_weight > 0), given as what `set_ewc` takes: a pair
    (source_state, fisher) of {name: tensor} mappings, fisher None for the L2-SP penalty.  `patch_heads`: the
    rick_amd.patchd.PatchHeads of CDC's patch-level discriminator (cfg.subspace_freq > 0; built here when None).  Deviation from
    CDC as recalled: R1 stays on the image-level logits, where CDC sends it through the patch head on patch iterations.
    `clip`: the rick_amd.clipguide.ClipGuide (encoder and direction) of the CLIP-space terms; never used while they are off."""

    def __init__(self, cfg, generator, discriminator, g_ema, d_ema, dp=None, g_source=None, ewc=None, d_source=None,
                 patch_heads=None, clip=None):
        self.cfg, self.g, self.d, self.g_ema, self.d_ema, self.dp = cfg, generator, discriminator, g_ema, d_ema, dp
        # the discriminator-side augmentation: DiffAugment (cfg.diffaug) or ADA (cfg.augment), never both; None when both are off
        self._augmenter = AdaAugmenter(self) if cfg.augment else None
        if cfg.diffaug:
            self._augmenter = DiffAugmenter(self, cfg.diffaug)
            if cfg.augment:
                raise ValueError('RickTrainer: augment (ADA) and diffaug are alternatives; set one of them')
        self.device = next(generator.parameters()).device
        self.g_source, self.d_source, self.clip = g_source, d_source, clip
        if cfg.ewc_weight < 0 or not math.isfinite(cfg.ewc_weight):
            raise ValueError('RickTrainer: ewc_weight must be finite and >= 0')
        if cfg.ewc_weight > 0 and ewc is None:
            raise ValueError('RickTrainer: ewc_weight > 0 needs the anchor (ewc=(source_state, fisher))')
        if isinstance(cfg.kml_rank, bool) or not isinstance(cfg.kml_rank, int) or not 0 <= cfg.kml_rank <= 8:
            raise ValueError('RickTrainer: kml_rank must be an integer in 0 ... 8')
        if cfg.svd_adapt and cfg.kml_rank > 0:
            raise ValueError('RickTrainer: svd_adapt and kml_rank > 0 are alternatives (both rewrite the frozen weights)')
        if cfg.svd_adapt and cfg.warmup_iter > 0:
            raise ValueError('RickTrainer: svd_adapt needs warmup_iter = 0 (the warm-up stage switches D\'s gradients off layer by '
                             'layer; singular-value adaptation has no such stage)')
        if cfg.dcl_d_weight < 0 or not math.isfinite(cfg.dcl_d_weight):
            raise ValueError('RickTrainer: dcl_d_weight must be finite and >= 0')
        if not cfg.dcl_tau > 0 or not math.isfinite(cfg.dcl_tau):         # the temperature of both contrastive terms
            raise ValueError('RickTrainer: dcl_tau must be finite and > 0')
        if cfg.dcl_d_weight > 0 and (g_source is None or d_source is None):
            raise ValueError('RickTrainer: dcl_d_weight > 0 needs the frozen source generator and discriminator (g_source=, d_source=)')
        if cfg.dcl_d_weight > 0 and (cfg.augment or cfg.diffaug):
            raise ValueError('RickTrainer: dcl_d_weight > 0 together with augment or diffaug is not supported (the source-side image '
                             "would have to be augmented with the fake's draw)")
        for name, src, net in (('g_source', g_source, generator), ('d_source', d_source, discriminator)):
            if src is None:
                continue
            if src is net:
                raise ValueError(f'RickTrainer: {name} must be a copy of the source network, not the network being trained')
            if next(src.parameters()).device != self.device:
                raise ValueError(f'RickTrainer: {name} on {next(src.parameters()).device}, generator on {self.device}')
            src.eval()
            for p in src.parameters():
                p.requires_grad = False
        self.g_terms = gterms.build(self)       # the G step's extra loss terms that are on (rick_amd/gterms.py)
        if isinstance(cfg.subspace_freq, bool) or not isinstance(cfg.subspace_freq, int) or cfg.subspace_freq < 0:
            raise ValueError('RickTrainer: subspace_freq must be an integer >= 0')
        if cfg.subspace_freq > 0:
            from . import patchd
            if dp is not None:
                raise ValueError('RickTrainer: subspace_freq > 0 together with data parallelism (dp=) is not supported (the '
                                 "exchange of the heads' gradients is not built)")
            if cfg.dcl_d_weight > 0:
                raise ValueError('RickTrainer: subspace_freq > 0 together with dcl_d_weight > 0 is not supported (the contrastive '
                                 'term needs the whole feature list, which a patch step that leaves the trunk early does not '
                                 'have: not built)')
            if cfg.n_anchors < 1 or not cfg.subspace_std >= 0 or not math.isfinite(cfg.subspace_std):
                raise ValueError('RickTrainer: n_anchors must be >= 1 and subspace_std finite and >= 0')
            if patch_heads is None:
                patch_heads = patchd.PatchHeads().to(self.device)
            n_taps = len(patchd.patch_taps(discriminator, patch_heads.channels))
            if not 1 <= cfg.feat_ind <= min(n_taps, len(patch_heads.new_conv)):
                raise ValueError(f'RickTrainer: feat_ind {cfg.feat_ind} with {n_taps} patch taps in the discriminator and '
                                 f'{len(patch_heads.new_conv)} heads')
            if next(patch_heads.parameters()).device != self.device:
                raise ValueError(f'RickTrainer: patch_heads on {next(patch_heads.parameters()).device}, generator on {self.device}')
        elif patch_heads is not None:
            raise ValueError('RickTrainer: patch_heads given with subspace_freq = 0')
        # packed conv weights: one refresh launch per network
        self._pack_groups = [op.register_pack_group(net) for net in (generator, discriminator)]
        self._ema_pack_groups = [op.register_pack_group(net) for net in (g_ema, d_ema)]
        self.g_flat = FlatParams(generator.named_parameters(), g_optim_filter)
        self.d_flat = FlatParams(discriminator.named_parameters(), d_optim_filter)
        self.g_ema_flat = FlatParams(g_ema.named_parameters())
        self.d_ema_flat = FlatParams(d_ema.named_parameters())
        g_ratio = cfg.g_reg_every / (cfg.g_reg_every + 1)
        d_ratio = cfg.d_reg_every / (cfg.d_reg_every + 1)
        self.g_optim = MaskedFlatAdam(self.g_flat, cfg.lr * g_ratio, (0 ** g_ratio, 0.99 ** g_ratio))
        self.d_optim = MaskedFlatAdam(self.d_flat, cfg.lr * d_ratio, (0 ** d_ratio, 0.99 ** d_ratio))
        # parameters no optimiser owns never need gradients in the train steps
        for n, p in generator.named_parameters():
            p.requires_grad = g_optim_filter(n)
        self._d_all = dict(discriminator.named_parameters())
        self.mean_path_length = 0
        self.idx_freeze_g = self.idx_freeze_d = None
        self.zero_idx_g = self.zero_idx_d = None
        self.losses = {}
        self.use_graphs = False
        self.step_events = None     # list of (step name, event) while bench.py times step types
        self._gs, self._inject, self._layer_idx, self._real = {}, {}, None, None
        self._fisher_state = None   # persistent accumulators / static inputs / captured per-sample graph of the Fisher sweep
        self._pending = None        # (graph state, flat, optimiser, optimiser graph) of a step whose gradient exchange is in flight
        # adaptive discriminator augmentation (cfg.augment): p, the device sign sum of D's real logits and the D step's augmented
        # reals (`_aug_real`, the R1 step's input).  The persistent device parameter blocks of the steps are the augmenter's: each
        # step's `pre=` hook refills its block, captured graphs read it.  `aug_source(n)`, when set, returns the (G, C) of a call of
        # n images instead of the sampler, `diffaug_source(n)` DiffAugment's parameter records (tests pin the draws with them).
        self.ada = AdaController(cfg)
        self.aug_source = self.diffaug_source = None
        self._ada_sum = torch.zeros((), device=self.device) if cfg.augment and self.ada.adaptive else None
        if dp is not None:
            dp.attach(self.g_flat, self.d_flat)
        # the slice adapters (rick_amd/adapter.py): kernel modulation of the frozen filters (cfg.kml_rank > 0) or singular-value
        # adaptation (cfg.svd_adapt), one per network, stepped with the network's lr / betas.  With svd_adapt the networks' own
        # optimisers get its freeze mask (RICK's Fisher masks and this mask are alternatives: fisher_sweep refuses)
        nets = ((self.g_flat, self.g_optim), (self.d_flat, self.d_optim))
        self._adapters, self._adapted_by = {}, None         # FlatParams -> its adapter; what the messages call the feature
        self.kml_g = self.kml_d = self.svd_g = self.svd_d = None
        if cfg.kml_rank > 0:
            from . import kml
            self._adapted_by = 'kernel modulation (kml_rank > 0)'
            self._adapters = {flat: kml.KmlState(flat, cfg.kml_rank, lr=optim.lr, betas=optim.betas) for flat, optim in nets}
            self.kml_g, self.kml_d = self._adapters.values()
        if cfg.svd_adapt:
            from . import svd
            self._adapted_by = 'singular-value adaptation (svd_adapt)'
            self._adapters = {flat: svd.SvdAdapter(flat, lr=optim.lr, betas=optim.betas) for flat, optim in nets}
            self.svd_g, self.svd_d = self._adapters.values()
            for flat, optim in nets:
                optim.set_mask(self._adapters[flat].frozen_mask(rest=cfg.svd_train_rest))
        # CDC's patch-level discriminator and anchor sampling (rick_amd/patchd.py): the heads' parameters in a FlatParams of their
        # own with a MaskedFlatAdam at D's learning rate and betas (the arrangement FlatAdapter has for its factors), stepped
        # with D's optimiser on patch D steps only: no masks, no EMA copy, no part in the Fisher sweep.  `anchors` may be set.
        self.patch_heads, self.anchors, self.last_patch = patch_heads, None, None
        self.head_flat = self.head_optim = None
        if cfg.subspace_freq > 0:
            self._head_pack = op.register_pack_group(patch_heads)
            self.head_flat = FlatParams(patch_heads.named_parameters())
            self.head_optim = MaskedFlatAdam(self.head_flat, self.d_optim.lr, tuple(self.d_optim.betas))
            self.anchors = torch.randn(cfg.n_anchors, cfg.latent, device=self.device)
        self.ewc = None
        if ewc is not None:
            self.set_ewc(*ewc) if isinstance(ewc, (tuple, list)) else self.set_ewc(ewc)

    # ---- elastic weight consolidation (rick_amd/ewc.py)
    def set_ewc(self, source_state, fisher=None):
        """Build the anchor of the EWC term on the generator's flat buffer (FlatParams has re-homed the parameters, so it can only
        be built once the trainer exists): `source_state` {name: tensor} (the source generator's state_dict), `fisher` {name:
        tensor} (ewc.estimate_fisher) or None for all ones.  An EwcAnchor built on this trainer's g_flat is taken as it is.
        Captured steps are dropped: they read the previous anchor's buffers."""
        from .ewc import EwcAnchor
        if isinstance(source_state, EwcAnchor):
            if source_state.flat is not self.g_flat:
                raise ValueError("RickTrainer.set_ewc: the anchor must be built on this trainer's g_flat")
            anchor = source_state
        else:
            anchor = EwcAnchor(self.g_flat, source_state, fisher)
        if self.ewc is not None:
            self.invalidate_graphs()
        self.ewc = anchor
        return anchor

    def _ewc_term(self):
        """MaskedFlatAdam.before_step of the G step: the averaged gradient is complete (every rank adds the identical term to the
        identical gradient) and Adam is next; in the split data-parallel capture this lands in the optimiser graph."""
        from .ewc import penalty_
        a, mask = self.ewc, self.g_optim.mask
        value = penalty_(a, self.cfg.ewc_weight, None if mask is None else mask[a.lo:a.hi])
        self.losses['ewc'] = value.detach()     # a new alias of the anchor's result tensor: registered as an output of a capture

    # ---- the slice adapters (rick_amd/adapter.py)
    def _adapter(self, flat):
        """The adapter whose grads_ / adam_step / apply_ bracket the network's optimiser step in _run: KML's or FSGAN's (never
        both), None without one."""
        return self._adapters.get(flat)

    def _no_graphs(self, how):
        raise RuntimeError(f'RickTrainer: {how} with {self._adapted_by} is not supported')

    def kml_rows_from_masks(self):
        """Flag "frozen and not pruned" on every modulated layer, from the index sets the masks were built from (idx_freeze_*,
        zero_idx_*).  Called when a Fisher sweep installs new masks; a no-op without KML."""
        for kml, freeze, zero in ((self.kml_g, self.idx_freeze_g, self.zero_idx_g), (self.kml_d, self.idx_freeze_d, self.zero_idx_d)):
            if kml is not None:
                kml.set_rows_from_index_sets(freeze, zero)

    # ---- gradient flags of the discriminator for the current stage (:202-211)
    def _set_d_stage(self, i):
        warm = i < self.cfg.warmup_iter
        for n, p in self._d_all.items():
            p.requires_grad = (('final' in n) if warm else True) and d_optim_filter(n)

    def _d_frozen(self, extra=()):
        """requires_grad off on every parameter of D (and of `extra`) inside the context."""
        class _Ctx:
            def __init__(s, params):
                s.params, s.flags = params, None

            def __enter__(s):
                s.flags = [p.requires_grad for p in s.params]
                for p in s.params:
                    p.requires_grad = False

            def __exit__(s, *a):
                for p, f in zip(s.params, s.flags):
                    p.requires_grad = f
        return _Ctx(list(self._d_all.values()) + list(extra))

    def _reduce(self, flat):
        if self.dp is not None:
            self.dp.all_reduce(flat)

    def _sink(self):
        """op.grad_sink() — except in the eager data-parallel mode, whose bucket all-reduces are launched from the
        parameters' post-accumulate-grad hooks while backward is still running: a sunk gradient fires no hook, so every
        bucket with a conv weight would only leave at the end of backward and nothing would overlap."""
        import contextlib
        if self.dp is not None and getattr(self.dp, 'hooks_enabled', False) and getattr(self.dp, 'active', getattr(self.dp, 'world', 1) > 1):
            return contextlib.nullcontext()
        return op.grad_sink()

    def _zero_grad(self, flat):
        flat.zero_grad()
        if self.dp is not None:
            self.dp.prepare(flat)          # bucket counts follow the stage's requires_grad flags

    # ---- hipGraph replay of whole steps ------------------------------------------------------------------
    # One RICK iteration is ~2 500 kernel launches issued from Python autograd; measured on MI355X the host needs
    # longer to ENQUEUE an iteration (34.8 ms) than the GPU needs to run it, so the loop was host-bound.  With
    # `use_graphs` every step type (D, R1, G, path length) is captured once — forward, backward, weight re-packing
    # and the masked Adam with its device-side step counters — and replayed afterwards; per-step host randomness
    # (style-mixing index) is written into device scalars before the replay.  With data parallelism the capture is
    # split around the gradient all-reduce (forward/backward graph -> RCCL -> optimiser graph).
    def enable_graphs(self, on=True):
        if on and self._adapters:
            self._no_graphs('hipGraph replay')
        self.use_graphs = bool(on)
        if self.dp is not None:
            self.dp.hooks_enabled = not self.use_graphs      # a replayed backward runs no Python hooks
        if on:
            for opt in (self.g_optim, self.d_optim):         # the mask buffer must exist before a launch is captured
                if opt.mask is None:
                    opt.mask = torch.zeros(opt.fp.total, dtype=torch.uint8, device=self.device)

    def prepare_graphs(self, real_img):
        """Capture all four step graphs up front (two eager warm-up calls + the capturing call of each step type), so
        that no capture lands inside a timed region.  These are real training steps."""
        if not self.use_graphs:
            return
        if self._real is None:
            self._real = torch.empty_like(real_img)
        self._real.copy_(real_img)
        for _ in range(3):
            self.d_step(self._real, None, graph=True)
            self.r1_step(self._aug_real if self.cfg.augment else self._real, graph=True)
            self.g_step(None, graph=True)
            self.plr_step(None, graph=True)
            self.ema_step()

    def _draw_inject(self, key):
        """Host side of mixing_noise + Generator.forward's random inject_index (:130-135, model_probe_tune.py:555-560):
        with probability `mixing` two latents, switched at a uniform layer index in [1, n_latent-1]; otherwise one
        latent for every layer (inject = n_latent).  Written to a device scalar the captured graph reads."""
        n_latent = self.g.n_latent
        k = random.randint(1, n_latent - 1) if (self.cfg.mixing > 0 and random.random() < self.cfg.mixing) else n_latent
        t = self._inject.get(key)
        if t is None:
            t = self._inject[key] = torch.zeros((), dtype=torch.int64, device=self.device)
            self._layer_idx = torch.arange(n_latent, device=self.device).view(1, -1, 1)
        t.fill_(k)
        self._advance_latent_pool(key)

    # The mapping network is frozen (the optimiser owns none of its parameters, train_dynamic_update_prune.py:908-917) and its
    # input is fresh noise: the W-space rows of the next LATENT_POOL steps of a step type are i.i.d. draws that do not depend
    # on anything the training changes.  They are computed LATENT_POOL steps at a time by ONE pass through the 8 layers (eagerly,
    # between graph replays) and a step's graph gathers its rows by a device-side index — instead of a randn + 8 mapping-layer
    # launches of ~9-12 us inside every D, G and path-length step (0.2 ms of an iteration).
    LATENT_POOL = 16

    def _pool_ok(self):
        return self.LATENT_POOL > 1 and not os.environ.get('RICK_NO_LATENT_POOL') and not any(
            p.requires_grad for p in self.g.style.parameters())

    def _style_stamp(self):
        """What the pooled rows are valid for: the mapping network's weights as loaded (load_state_dict copies in place and
        bumps _version; the optimiser never touches them)."""
        return tuple((None if p.is_inference() else p._version, p.data_ptr()) for p in self.g.style.parameters())

    def _fill_latent_pool(self, ent):
        with torch.no_grad():
            z = torch.randn(self.LATENT_POOL * ent['rows'], self.cfg.latent, device=self.device)
            ent['w'].copy_(self.g.style(z).view(self.LATENT_POOL, ent['rows'], -1))
        ent['stamp'] = self._style_stamp()

    def _advance_latent_pool(self, key):
        """Host side, before a step's graph runs (with _draw_inject): point the step at the next pool row, refill when used up."""
        ent = getattr(self, '_lat_pool', {}).get(key)
        if ent is None:
            return
        ent['pos'] += 1
        if ent['pos'] >= self.LATENT_POOL or ent.get('stamp') != self._style_stamp():
            # used up — or the mapping network was reloaded (checkpoint.resume / load_source on a trainer that has already
            # stepped): rows computed with the old weights are not draws of the current model
            self._fill_latent_pool(ent)
            ent['pos'] = 0
        ent['idx'].fill_(ent['pos'])

    def _graph_latents(self, key, batch):
        """[batch, n_latent, 512] W-space latents with the style switch applied on the device (same values as the
        reference's cat of repeated w1 / w2 rows)."""
        if not self._pool_ok():
            z = torch.randn(2 * batch, self.cfg.latent, device=self.device)
            w = self.g.style(z).view(2, batch, 1, -1)
            return torch.where(self._layer_idx < self._inject[key], w[0], w[1])
        pools = self.__dict__.setdefault('_lat_pool', {})
        ent = pools.get(key)
        if ent is None or ent['rows'] != 2 * batch:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError('latent pool must exist before hipGraph capture (run the step eagerly once)')
            ent = pools[key] = dict(rows=2 * batch, pos=0, idx=torch.zeros(1, dtype=torch.int64, device=self.device),
                                    w=torch.empty(self.LATENT_POOL, 2 * batch, self.cfg.latent, device=self.device))
            self._fill_latent_pool(ent)
        w = ent['w'].index_select(0, ent['idx']).view(2, batch, 1, -1)
        return torch.where(self._layer_idx < self._inject[key], w[0], w[1])

    def _run(self, key, fb, flat, optim, pre=None, fb_head=None):
        """fb(): forward + backward into flat.grad;  then gradient exchange and optimiser step.

        fb_head(): an optional first part of the step that does not read the parameters the PREVIOUS step is still
        updating (the generator forward of the G step does not touch D).  Under data parallelism with step graphs the
        optimiser part of a step is deferred (`_pending`): its gradient buckets are launched right behind the replayed
        forward/backward graph and the step returns; the next step replays its head, THEN waits for the exchange, replays the
        pending optimiser graph and continues — the all-reduce of the D gradients travels while the generator forward
        runs (north star: "overlapped with the next micro-batch forward")."""
        adapter = self._adapter(flat)
        if adapter is not None and key is not None:
            self._no_graphs('a graph=True step')
        if pre is not None:
            pre()
        st = None
        if key is not None and self.use_graphs:
            st = self._gs.setdefault(key, {'n': 0})
            if 'graphs' in st and st['sig'] != self._graph_signature(optim):
                # optimiser state / stage changed under the capture: drop it AND run the two eager warm-up steps again —
                # a new requires_grad pattern needs new descriptor tables (PackGroup, ModulationBank), which must not be
                # built inside a capture
                self._finish_pending()
                del st['graphs']
                st['n'] = 0
            st['n'] += 1
        if st is None or st['n'] <= 2:                        # eager (also the warm-up of a graph: caches, allocator)
            self._finish_pending()
            if fb_head is not None:
                fb_head()
            fb()
            self._reduce(flat)
            if adapter is not None:                           # the averaged gradient: da / db (dd) are identical on every rank
                adapter.grads_()
            optim.step()                                      # (the freeze bit leaves the adapted weights alone)
            if adapter is not None:
                adapter.adam_step()
                adapter.apply_()
            return
        split = self.dp is not None and getattr(self.dp, 'active', True)
        if 'graphs' not in st:
            self._finish_pending()
            # packed weights are refreshed on the HOST side of the graphs: a network is repacked once per update of its
            # weights (the D step's graph used to repack G again although the G step's graph had just done so, and vice versa)
            for grp in self._pack_groups:
                grp.refresh()
            torch.cuda.synchronize()
            before = list(optim.steps)
            seen = dict(self.losses)
            if not split:
                g = torch.cuda.CUDAGraph()
                with self._capture(g):
                    if fb_head is not None:
                        fb_head()
                    fb()
                    optim.step()
                st['graphs'] = (None, g, None)
            else:
                # head | forward/backward | optimiser as separate graphs from ONE memory pool: the autograd graph the head
                # builds (saved activations in pool memory) is consumed by the backward captured in the second graph
                gh = torch.cuda.CUDAGraph() if fb_head is not None else None
                g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
                pool = None
                if gh is not None:
                    with self._capture(gh):
                        fb_head()
                    pool = gh.pool()
                with self._capture(g1, pool=pool):
                    fb()
                with self._capture(g2, pool=g1.pool()):
                    optim.step()
                st['graphs'] = (gh, g1, g2)
            st['runs'] = list(optim.last_runs)
            st['losses'] = {k: v for k, v in self.losses.items() if seen.get(k) is not v}   # this graph's output tensors
            optim.steps[:] = before                           # capture executes nothing: the replay below is this step
            st['sig'] = self._graph_signature(optim)
        gh, g1, g2 = st['graphs']
        if not split:
            for grp in self._pack_groups:
                grp.refresh()
            g1.replay()
            self._after_optimizer(st, flat, optim)
            return
        if gh is not None:
            # The head may only run ahead of a pending step that updates a DIFFERENT network (the generator forward while
            # D's buckets travel).  A pending step on the head's own parameters (two G steps in a row through the step API)
            # must land first: the head would otherwise read pre-update weights that the backward then no longer matches,
            # and its replay would run before the optimiser graph captured behind it in the shared memory pool.
            if self._pending is not None and self._pending[1] is flat:
                self._finish_pending()
            for grp in self._pack_groups:                     # (the head only reads networks no pending step is updating)
                grp.refresh(skip=self._pending_params())
            gh.replay()                                       # ... while the previous step's buckets are on the wire
        self._finish_pending()
        for grp in self._pack_groups:
            grp.refresh()
        g1.replay()
        self.dp.launch(flat)
        self._pending = (st, flat, optim, g2)

    def _capture(self, graph, pool=None):
        """torch.cuda.graph(...) — with a process group alive, in 'thread_local' capture-error mode: RCCL's watchdog thread
        polls its events (hipEventQuery) at any time, and under the default 'global' mode such a call from ANOTHER thread
        while this one is capturing is an error that takes the process down (hipErrorStreamCaptureUnsupported: seen on
        MI355X with one rank; it is a timing matter, so it would have surfaced on some rank of an 8-GPU run)."""
        import torch.distributed as dist
        mode = 'thread_local' if (dist.is_available() and dist.is_initialized()) else 'global'
        return torch.cuda.graph(graph, pool=pool, capture_error_mode=mode)

    def _pending_params(self):
        return None if self._pending is None else self._pending[1]

    def _finish_pending(self):
        """Complete a step whose optimiser part was deferred: wait for its gradient exchange, replay its optimiser graph."""
        if self._pending is None:
            return
        st, flat, optim, g2 = self._pending
        self._pending = None
        self.dp.wait(flat)
        g2.replay()
        self._after_optimizer(st, flat, optim)

    def _after_optimizer(self, st, flat, optim):
        optim.last_runs = st['runs']
        optim.note_replayed_step()
        # the replay updated the parameters through raw pointers: packed weights are stale (a host-side counter; the next
        # _run / fisher_sweep refreshes the pack group before it replays anything)
        op.bump_weights_epoch(flat.params)
        self.losses.update(st['losses'])                      # eager steps in between may have re-bound the entries

    def _graph_signature(self, optim):
        """What a captured step bakes in from the host: which parameters step (requires_grad pattern of the stage) and
        how they group into runs of equal step count (one bias-correction row per run).  A checkpoint resume or a
        stage change alters it; the step is then re-captured instead of replayed with stale grouping."""
        fp = optim.fp
        active = tuple(fp.params[i].requires_grad for i in fp.opt_idx)
        st = [optim.steps[i] for i in fp.opt_idx]
        rel = tuple(s - st[0] for s in st)
        # (+ whether the step gathers its latents from the pool: mapping-network parameters that become trainable after a
        # capture switch the step back to drawing and mapping its own noise)
        # (+ the EWC term of the G step: whether its two launches are part of the capture, and the weight they carry)
        return (active, rel, optim.lr, tuple(optim.betas), optim.eps, self._pool_ok(), self.cfg.ewc_weight > 0,
                float(self.cfg.ewc_weight))

    def invalidate_graphs(self):
        """Drop every captured step (after loading a checkpoint or changing optimiser hyper-parameters)."""
        self._finish_pending()
        for st in self._gs.values():
            st.pop('graphs', None)
            st['n'] = 0                                       # two eager warm-up steps before the next capture
        self._fisher_state = None
        self.__dict__.pop('_lat_pool', None)                  # pooled W rows belong to the weights they were mapped with

    # ---- adaptive discriminator augmentation
    @property
    def ada_p(self):
        return self.ada.p

    @ada_p.setter
    def ada_p(self, v):
        self.ada.p = float(v)

    def _ada_after_d_step(self, batch):
        """Adaptive p (train_dynamic_update_prune.py:440-459) after a D step of `batch` images on this rank."""
        if self._ada_sum is None:
            return
        world = getattr(self.dp, 'world', 1) if self.dp is not None else 1
        if not self.ada.due(batch * world):
            return
        stat = self._ada_sum.view(1).clone()
        if self.dp is not None and world > 1:
            self.dp.all_reduce_vectors([stat])
        self.ada.update(float(stat))
        self._ada_sum.zero_()

    # ---- steps (each returns the loss tensor; no host sync)
    def d_step(self, real_img, noise, i=10 ** 9, g_noise=None, graph=False, dcl_layers=None, dcl_inject=None, patch=None):
        """Logistic D step.  With cfg.dcl_d_weight > 0 the discriminator contrastive term (rick_amd/dcl.py) is added before the one
        backward(): anchors and negatives are the two halves of the feature list the pass over cat(fake, real) returns anyway, the
        positives come from one no-grad pass G_s -> D_s with the mixing index and noise maps of the fakes (drawn here, handed to
        both generators).  Its drawn layers change the launch list, so such a step is never captured: `graph=True` then runs the
        eager path, as g_step does with the distance-consistency term.  `dcl_layers` and `dcl_inject` fix the draws (tests);
        `g_noise` fixes the noise maps.  With cfg.subspace_freq > 0 (rick_amd/patchd.py) the step also runs eagerly under
        `graph=True`; `patch=p_ind` then sends cat(fake, real) through patchd.patch_logits at that tap instead of the whole
        discriminator — the logistic loss over every entry of the two patch maps — and steps the heads' own Adam with D's; the
        augmentation seam applies to the images as on image-level steps, ADA's controller is left alone.  Parameters behind
        the exit get no gradient from autograd; their slices of the flat gradient stay zero and Adam (beta1 = 0) leaves them
        bit for bit, as it does the heads of the other taps."""
        self._set_d_stage(i)
        dcl_on = self.cfg.dcl_d_weight > 0
        patch_on = self.cfg.subspace_freq > 0
        if patch is not None and not patch_on:
            raise ValueError('RickTrainer.d_step: patch= needs cfg.subspace_freq > 0')
        if (dcl_on or patch_on) and graph:
            graph = False
            if noise is None:
                noise = mixing_noise(real_img.shape[0], self.cfg.latent, self.cfg.mixing, self.device)
        key = 'd' if graph else None
        batch = real_img.shape[0]

        aug, ada = self._augmenter, self.cfg.augment

        def fb():
            with torch.no_grad():
                if graph:
                    fake_img, _ = self.g([self._graph_latents(key, batch)], input_is_latent=True, noise=g_noise)
                elif dcl_on:
                    inject, maps = self._dcl_d_draws(noise, g_noise, dcl_inject)
                    fake_img, _ = self.g(noise, noise=maps, inject_index=inject)
                    feats_pos = self.d_source(self.g_source(noise, noise=maps, inject_index=inject)[0])[1]
                else:
                    fake_img, _ = self.g(noise, noise=g_noise)
                x = torch.cat([fake_img, real_img], 0)
                if aug:                          # augment(real), augment(fake) of the reference: one launch pair over cat(fake, real)
                    x = aug.apply(x, aug.blocks['d'].dev)
                    if ada:                      # the R1 step's input (a static buffer under graphs)
                        self._aug_real.copy_(x[batch:])
            # one pass over cat(fake, real): identical to the reference's two calls (per-call minibatch-stddev
            # statistics are kept), half the launches and twice the GEMM rows per launch
            with self._sink():                   # conv weight gradients are added straight into the flat buffer
                if patch is not None:
                    from . import patchd
                    pred = patchd.patch_logits(self.d, self.patch_heads, x, patch)
                    self.head_flat.zero_grad()
                else:
                    pred, feats = self.d(x, calls=2)
                fake_pred, real_pred = pred.chunk(2, 0)
                d_loss = d_logistic_loss(real_pred, fake_pred)
                total = d_loss
                if dcl_on:
                    from . import dcl
                    nf = fake_img.shape[0]
                    layers = dcl_layers if dcl_layers is not None else dcl.draw_d_layers(len(feats), nf)
                    dcl_loss = dcl.discriminator_contrastive_loss([f[:nf] for f in feats], feats_pos, [f[nf:] for f in feats],
                                                                  layers, self.cfg.dcl_tau)
                    total = d_loss + self.cfg.dcl_d_weight * dcl_loss
                    self.losses['dcl_d'] = dcl_loss.detach()
                if self._ada_sum is not None and patch is None:
                    self._ada_sum.add_(torch.sign(real_pred.detach()).sum())
                self._zero_grad(self.d_flat)
                # bias / noise-strength sums: one second-stage launch for the whole pass; (RICK_WGRAD_OVERLAP=1: sunk weight
                # gradients on a second stream next to the data-gradient chain — measured slower, off by default, op/conv.py)
                with op.deferred_sums(), op.wgrad_overlap():
                    total.backward()
            self.losses.update(d=d_loss.detach(), real_score=real_pred.detach().mean(), fake_score=fake_pred.detach().mean())

        def pre():
            if graph:
                self._draw_inject(key)
            if aug:
                if ada and (getattr(self, '_aug_real', None) is None or self._aug_real.shape != real_img.shape):
                    self._aug_real = torch.empty_like(real_img)
                # the reference draws real's parameters first, then fake's; the launch runs over cat(fake, real)
                aug.prepare('d', 2, batch, reverse=True)
        self._run(key, fb, self.d_flat, self.d_optim, pre=pre if (graph or aug) else None)
        if patch is not None:
            self.head_optim.step()
        else:
            self._ada_after_d_step(batch)
        return self.losses['d']

    def r1_step(self, real_img, i=10 ** 9, graph=False):
        cfg = self.cfg
        self._set_d_stage(i)
        aug = None if cfg.augment else self._augmenter          # ADA: the caller passes the D step's augmented reals (_aug_real)
        batch = real_img.shape[0]

        def fb():
            real = real_img.detach().requires_grad_(True)
            with op.second_order():
                # DiffAugment (the convention of its authors' StyleGAN2 trainer): D sees a fresh draw of the augmented reals, the
                # penalty is on the gradient w.r.t. the PLAIN reals — adjoint in the inner gradient, forward without offset in its
                # backward
                real_pred, _ = self.d(aug.apply(real, aug.blocks['r1'].dev) if aug else real)
                real_pred = real_pred.view(real.size(0), -1).mean(dim=1).unsqueeze(1)
                r1_loss = d_r1_loss(real_pred, real)
                self._zero_grad(self.d_flat)
                (cfg.r1 / 2 * r1_loss * cfg.d_reg_every + 0 * real_pred[0]).backward()
            self.losses['r1'] = r1_loss.detach()
        self._run('r1' if graph else None, fb, self.d_flat, self.d_optim,
                  pre=(lambda: aug.prepare('r1', 1, batch)) if aug else None)
        return self.losses['r1']

    def _feature_pair(self, z, g_noise=None):
        """The feature lists of one latent batch z through the generator being trained and through the frozen source generator
        (no grad): (feats_t, feats_s).  `g_noise`: fixed noise maps for both generators (drawn per call otherwise)."""
        with torch.no_grad():
            _, feats_s = self.g_source([z], noise=g_noise, return_feats=True)
        _, feats_t = self.g([z], noise=g_noise, return_feats=True)
        return feats_t, feats_s

    def _dcl_d_draws(self, noise, g_noise, inject=None):
        """The draws Generator.forward would make for the fakes of a D step, made here so that the generator being trained and the
        frozen source generator get the same ones: the style-mixing index (None for a single latent) and the noise maps."""
        if len(noise) < 2:
            inject = None
        elif inject is None:
            inject = random.randint(1, self.g.n_latent - 1)
        if g_noise is None:
            B = noise[0].shape[0]
            res = [4] + [2 ** k for k in range(3, self.g.log_size + 1) for _ in range(2)]
            flat = torch.empty(B * sum(r * r for r in res), device=self.device, dtype=torch.float32).normal_()
            g_noise, o = [], 0
            for r in res:
                g_noise.append(flat[o:o + B * r * r].view(B, 1, r, r))
                o += B * r * r
        return inject, g_noise

    def g_step(self, noise, g_noise=None, graph=False, patch=None, **draws):
        """Non-saturating G step.  The extra loss terms that are on (`g_terms`, rick_amd/gterms.py) are added before the one
        backward(); `draws` are the keywords those terms declare to fix their random draws (tests), `g_noise` also fixes their
        noise maps; a keyword of a term that is off is ignored, one that no term declares is a TypeError.  A term whose launch list
        changes from step to step is not capturable: `graph=True` then runs the eager path (its own mixing noise, no step graph)
        while every other step type keeps replaying, and so does every G step with cfg.subspace_freq > 0 (rick_amd/patchd.py):
        `patch=p_ind` takes the non-saturating loss over the patch map of patchd.patch_logits at that tap; neither the
        discriminator nor the heads get gradients."""
        for k in draws:
            if k not in gterms.DRAWS:
                raise TypeError(f"RickTrainer.g_step() got an unexpected keyword argument '{k}'")
        patch_on = self.cfg.subspace_freq > 0
        if patch is not None and not patch_on:
            raise ValueError('RickTrainer.g_step: patch= needs cfg.subspace_freq > 0')
        if (patch_on or not all(t.capturable for t in self.g_terms)) and graph:
            graph = False
            if noise is None:
                noise = mixing_noise(self.cfg.batch, self.cfg.latent, self.cfg.mixing, self.device)
        key = 'g' if graph else None
        batch = self.cfg.batch
        box = {}

        def head():                              # generator forward: reads G only (D's update may still be in flight)
            with self._sink():
                if graph:
                    box['fake'], _ = self.g([self._graph_latents(key, batch)], input_is_latent=True, noise=g_noise)
                else:
                    box['fake'], _ = self.g(noise, noise=g_noise)

        aug = self._augmenter

        def fb():
            with self._sink(), self._d_frozen(self.patch_heads.parameters() if self.patch_heads is not None else ()):
                fake = box.pop('fake')
                if aug:                          # with gradients: the adjoint carries them back to G
                    fake = aug.apply(fake, aug.blocks['g'].dev)
                if patch is not None:
                    from . import patchd
                    fake_pred = patchd.patch_logits(self.d, self.patch_heads, fake, patch)
                else:
                    fake_pred, _ = self.d(fake)
                g_loss = g_nonsaturating_loss(fake_pred)
                total = g_loss
                memo = {}                        # what one term hands to a later one (a shared forward pair)
                for term in self.g_terms:
                    for name, (weight, value) in term(draws, g_noise, memo).items():
                        total = total + weight * value
                        self.losses[name] = value.detach()
                self._zero_grad(self.g_flat)
                with op.deferred_sums(), op.wgrad_overlap():
                    total.backward()
            self.losses['g'] = g_loss.detach()
        def pre():
            if graph:
                self._draw_inject(key)
            if aug:
                aug.prepare('g', 1, batch)
        # the EWC term is added at the top of the optimiser step: after the gradient exchange (the eager data-parallel mode still
        # has bucket all-reduces in flight when backward() returns), in the G step only (the path-length step has its own
        # optimiser step: the term there would be weighted 1 + 1 / g_reg_every times)
        if self.cfg.ewc_weight > 0:
            if self.ewc is None:
                raise ValueError('RickTrainer: ewc_weight > 0 needs the anchor (set_ewc)')
            self.g_optim.before_step = self._ewc_term
        try:
            self._run(key, fb, self.g_flat, self.g_optim, pre=pre if (graph or aug) else None, fb_head=head)
        finally:
            self.g_optim.before_step = None
        return self.losses['g']

    def _mixed_latents(self, noise):
        """W-space latents [B, n_latent, 512] for a list of 1 or 2 z tensors — Generator.forward's own mixing
        (random inject_index, model_probe_tune.py:555-560)."""
        n_latent = self.g.n_latent
        w = [self.g.style(z) for z in noise]
        if len(w) < 2:
            return w[0].unsqueeze(1).repeat(1, n_latent, 1)
        k = random.randint(1, n_latent - 1)
        return torch.cat([w[0].unsqueeze(1).repeat(1, k, 1), w[1].unsqueeze(1).repeat(1, n_latent - k, 1)], 1)

    def plr_step(self, noise, pl_noise=None, g_noise=None, graph=False):
        return self._plr_step(noise, pl_noise, g_noise, graph)

    def _plr_step(self, noise, pl_noise, g_noise, graph):
        cfg = self.cfg
        key = 'plr' if graph else None
        batch = max(1, cfg.batch // cfg.path_batch_shrink)
        if not torch.is_tensor(self.mean_path_length):      # persistent device scalar, updated in place (graph-safe)
            self.mean_path_length = torch.full((), float(self.mean_path_length), device=self.device)

        def fb():
            # The path-length gradient is taken w.r.t. the latents.  The optimiser owns no parameter of the mapping
            # network (train_dynamic_update_prune.py:908-917), so the latents enter as a detached leaf: the
            # reference's backward through the 8-layer MLP only produces gradients that are discarded, here it
            # (and its double backward) is not run.  Conv-weight gradients are unchanged.
            with torch.no_grad():
                lat = self._graph_latents(key, batch) if graph else self._mixed_latents(noise)
            lat = lat.detach().requires_grad_(True)
            with op.second_order():
                fake_img, latents = self.g([lat], input_is_latent=True, return_latents=True, noise=g_noise)
                path_loss, new_mean, path_lengths = g_path_regularize(fake_img, latents, self.mean_path_length,
                                                                      noise=pl_noise)
                self._zero_grad(self.g_flat)
                weighted = cfg.path_regularize * cfg.g_reg_every * path_loss
                if cfg.path_batch_shrink:
                    weighted = weighted + 0 * fake_img[0, 0, 0, 0]
                weighted.backward()
            self.mean_path_length.copy_(new_mean)
            self.losses.update(path=path_loss.detach(), path_length=path_lengths.detach().mean())
        self._run(key, fb, self.g_flat, self.g_optim, pre=(lambda: self._draw_inject(key)) if graph else None)
        return self.losses['path']

    def ema_step(self):
        """accumulate(g_ema, g), accumulate(d_ema, d) (:697-698) over ALL named parameters."""
        self._finish_pending()
        ema_flat(self.g_ema_flat, self.g_flat, self.cfg.ema_decay)
        ema_flat(self.d_ema_flat, self.d_flat, self.cfg.ema_decay)

    # ---- Fisher sweep (:214-393)
    def _fisher_sample(self, z, real, acc_g, acc_d, g_params, d_params, fixed_noise):
        """One sample of the sweep (:225-263): G / D forward at batch 1, both losses, grad^2 added to the accumulators."""
        fake, _ = self.g_ema([z.view(1, -1)], randomize_noise=not fixed_noise)
        fake_pred, _ = self.d_ema(fake)
        real_pred, _ = self.d_ema(real.view(1, 3, self.cfg.size, self.cfg.size))
        g_loss = g_nonsaturating_loss(fake_pred)
        d_loss = d_logistic_loss(real_pred, fake_pred)
        acc_g.add(autograd.grad(g_loss, g_params, retain_graph=True, allow_unused=True))
        acc_d.add(autograd.grad(d_loss, d_params, allow_unused=True))

    def fisher_sweep(self, latents, reals, first, fixed_noise=False):
        """latents: list of [1,512] tensors for THIS rank's samples; reals: matching [1,3,H,W].

        A sample is ~1 500 batch-1 launches issued through Python autograd — host-bound (21.5 ms per sample measured, of
        which the GPU works less than half).  With `use_graphs` the per-sample body is captured once (second sample of the
        first sweep; the first runs eagerly so that every packed-weight request and descriptor table exists) and replayed
        with the sample copied into static input buffers; the grad^2 accumulators are persistent tensors the captured
        launches add into.  Same kernels on the same data as the eager loop.

        Returns the two PERSISTENT accumulators (scaled grad^2 per parameter): the next sweep zeroes and refills them in
        place — clone what must outlive it."""
        cfg = self.cfg
        if cfg.svd_adapt:
            raise RuntimeError('RickTrainer: fisher_sweep with singular-value adaptation (svd_adapt) is not supported: RICK\'s '
                               'freeze / prune masks and the adapter\'s mask are alternatives')
        self._finish_pending()
        requires_grad(self.g_ema, True)
        requires_grad(self.d_ema, True)
        g_named, d_named = list(self.g_ema.named_parameters()), list(self.d_ema.named_parameters())
        g_params, d_params = [p for _, p in g_named], [p for _, p in d_named]
        st = self._fisher_state
        # what a captured per-sample graph bakes in: arithmetic mode, image size, which parameters take gradients
        sig = (fixed_noise, op.get_precision(), cfg.size, tuple(p.requires_grad for p in g_params + d_params))
        if st is None or st['sig'] != sig:
            st = self._fisher_state = {'sig': sig, 'acc': (FisherAccumulator(g_named), FisherAccumulator(d_named)),
                                       'z': torch.empty(1, cfg.latent, device=self.device),
                                       'real': torch.empty(1, 3, cfg.size, cfg.size, device=self.device), 'runs': 0, 'graph': None}
        acc_g, acc_d = st['acc']
        acc_g.zero_()
        acc_d.zero_()
        for z, real in zip(latents, reals):
            if not self.use_graphs:
                self._fisher_sample(z, real, acc_g, acc_d, g_params, d_params, fixed_noise)
                continue
            st['z'].copy_(z.view(1, -1))
            st['real'].copy_(real.view(1, 3, cfg.size, cfg.size))
            if st['graph'] is None and st['runs'] >= 1:
                for grp in self._ema_pack_groups:
                    grp.refresh()
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with self._capture(graph):
                    self._fisher_sample(st['z'], st['real'], acc_g, acc_d, g_params, d_params, fixed_noise)
                st['graph'] = graph
            if st['graph'] is not None:
                for grp in self._ema_pack_groups:         # the EMA weights move every iteration: repack on the host side
                    grp.refresh()
                st['graph'].replay()
            else:
                self._fisher_sample(st['z'], st['real'], acc_g, acc_d, g_params, d_params, fixed_noise)
            st['runs'] += 1
        scale = 1.0 / (cfg.num_fisher_img * cfg.batch)                 # :266-269
        acc_g.scale_(scale)
        acc_d.scale_(scale)
        conv, fc = g_filter_fim(acc_g.acc)
        dfim = d_filter_fim(acc_d.acc)
        if self.dp is not None:                                        # samples are sharded over ranks
            self.dp.all_reduce_vectors(list(conv.values()) + list(fc.values()) + list(dfim.values()))
        to_np = lambda d: {k: v.detach().cpu().numpy() for k, v in d.items()}   # noqa: E731
        self.fim = (to_np(conv), to_np(fc), to_np(dfim))
        self.idx_freeze_g, _, prune_g = decide_g(self.fim[0], self.fim[1], cfg.fisher_quantile, cfg.prune_quantile)
        self.idx_freeze_d, _, prune_d = decide_d(self.fim[2], cfg.fisher_quantile, cfg.prune_quantile)
        if first:
            self.zero_idx_g, self.zero_idx_d = prune_g, prune_d
        else:
            self.zero_idx_g = zero_idx_merge(self.zero_idx_g, prune_g)
            self.zero_idx_d = zero_idx_merge(self.zero_idx_d, prune_d)
        self.g_optim.set_mask(build_mask(self.g_flat, self.idx_freeze_g, self.zero_idx_g))
        self.d_optim.set_mask(build_mask(self.d_flat, self.idx_freeze_d, self.zero_idx_d))
        self.kml_rows_from_masks()
        return acc_g, acc_d

    # ---- one iteration in the reference's order (:395-589, 697-698)
    def iteration(self, i, real_img, fisher_inputs=None):
        cfg = self.cfg
        if fisher_inputs is not None and cfg.svd_adapt:
            raise RuntimeError('RickTrainer: iteration(fisher_inputs=...) with singular-value adaptation (svd_adapt) is not supported')
        if fisher_inputs is not None and i - cfg.warmup_iter >= 0 and (i - cfg.warmup_iter) % cfg.fisher_freq == 0:
            self.fisher_sweep(*fisher_inputs, first=(i == cfg.warmup_iter))
        graph = self.use_graphs and i >= cfg.warmup_iter      # the warm-up stage has its own requires_grad pattern
        if graph:
            if self._real is None:
                self._real = torch.empty_like(real_img)
            self._real.copy_(real_img)                        # captured launches read this buffer
            real_img = self._real
        nz = (lambda b: None) if graph else (lambda b: mixing_noise(b, cfg.latent, cfg.mixing, self.device))
        self._mark('begin')
        nz_dg, patch = nz, {}                                 # the noise and the extra arguments of the D and the G step
        if cfg.subspace_freq > 0:
            # CDC's schedule (rick_amd/patchd.py): an anchor iteration draws the latents of both steps from the anchor subspace and
            # keeps the image-level discriminator; the others use the patch path at one drawn tap in both steps
            from . import patchd
            which, p_ind = self.last_patch = patchd.draw_patch(i, cfg.subspace_freq, cfg.feat_ind)
            if which == 0:
                nz_dg = lambda b: [patchd.sample_anchor_latents(self.anchors, b, cfg.subspace_std)]     # noqa: E731
            else:
                patch = {'patch': p_ind}
        self.d_step(real_img, nz_dg(cfg.batch), i, graph=graph, **patch)
        self._mark('d')
        if i % cfg.d_reg_every == 0:       # with augmentation: the D step's augmented reals (:463-466)
            self.r1_step(self._aug_real if cfg.augment else real_img, i, graph=graph)
            self._mark('r1')
        if i >= cfg.warmup_iter:
            self.g_step(nz_dg(cfg.batch), graph=graph, **patch)
            self._mark('g')
            if i % cfg.g_reg_every == 0:
                self.plr_step(nz(max(1, cfg.batch // cfg.path_batch_shrink)), graph=graph)
                self._mark('plr')
        self.ema_step()
        self._mark('ema')

    def _mark(self, name):
        """bench.py's per-step-type timing: a HIP event on the launch stream after each step (no host sync).  Under data
        parallelism with step graphs the optimiser part of a step is deferred behind the next step's head (`_run`), so the
        event of step k is recorded before its all-reduce wait and optimiser graph have run: that time is charged to step
        k + 1 — per-step times of `--gpus N` runs are pipelined and not comparable with single-GPU ones;
        `ms_per_step` and `value` are unaffected (whole iterations, fenced)."""
        if self.step_events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.step_events.append((name, e))
