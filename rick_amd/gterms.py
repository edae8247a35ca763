"""The extra loss terms of the trainer's G step (rick_amd/train.py): distance consistency (rick_amd/cdc.py), DCL's generator
contrastive term CL1 (rick_amd/dcl.py) and the CLIP-space terms (rick_amd/clipguide.py).  RickTrainer calls `build` once and
keeps the terms that are switched on, in the order of TERMS; `g_step` adds what they return to the adversarial loss before its
one backward() and knows none of them by name.  A term class has

    weights              the config fields that weight its losses; the term is on when one of them is > 0
    draws                the keyword names g_step accepts for it: they pin the term's random draws (tests)
    capturable           False when the term's launch list changes from step to step: a G step with such a term runs eagerly
    check(cfg)           raises ValueError for a configuration that is wrong whether the term is on or off
    make(trainer)        None when the term is off; raises ValueError for a resource it lacks (g_source, the CLIP guide)
    term(draws, g_noise, memo) -> {loss name: (weight, unweighted loss tensor)}
                         `draws`: the keywords g_step was given; `g_noise`: fixed noise maps for every generator pass (drawn per
                         pass otherwise); `memo`: empty at the start of a step, what one term hands to a later one

A new term is one more class in TERMS."""
import math

import torch

from . import cdc, dcl


class GTerm:
    capturable = False      # all three draw layers or add forward passes of their own batch: no step graph fits the next step

    def __init__(self, trainer):
        self.tr = trainer
        if trainer.g_source is None:
            raise ValueError(f'RickTrainer: {" / ".join(self.weights)} > 0 needs the frozen source generator (g_source=)')

    @classmethod
    def check(cls, cfg):
        if any(getattr(cfg, w) < 0 or not math.isfinite(getattr(cfg, w)) for w in cls.weights):
            raise ValueError(f'RickTrainer: {" and ".join(cls.weights)} must be finite and >= 0')

    @classmethod
    def make(cls, trainer):
        return cls(trainer) if any(getattr(trainer.cfg, w) > 0 for w in cls.weights) else None


class FeaturePairTerm(GTerm):
    """One loss on the feature lists of one latent batch through the generator being trained and through the frozen source
    generator (RickTrainer._feature_pair) at one drawn layer per sample.  A subclass names its loss, its weight and batch fields,
    its smallest batch and its two draws (latents [batch, latent], layers) and supplies `loss`."""
    partner = None          # the later feature-pair term when two are on (`build`); _pair decides per step whether they share

    @classmethod
    def check(cls, cfg):
        super().check(cfg)
        if getattr(cfg, cls.batch) < cls.min_batch:
            raise ValueError(f'RickTrainer: {cls.batch} must be >= {cls.min_batch}')

    def rows(self, z):
        return z.shape[0] if z is not None else getattr(self.tr.cfg, self.batch)

    def __call__(self, draws, g_noise, memo):
        z, layers = (draws.get(k) for k in self.draws)
        if layers is None:      # one per sample of the pair: a pair that is shared has this term's own number of rows
            layers = cdc.draw_layers(self.tr.g.n_latent, self.rows(z))
        feats_t, feats_s = _pair(self, draws, g_noise, memo)
        return {self.name: (getattr(self.tr.cfg, self.weights[0]), self.loss(feats_t, feats_s, layers))}


def _pair(term, draws, g_noise, memo):
    """The forward pair (feats_t, feats_s) of a feature-pair term.  Two such terms share ONE pair when both are on, their batch
    sizes agree (a given latent tensor's row count wins over the config's) and they were not handed two different latent tensors;
    the shared latents are the first term's given ones, else the second's, else one draw.  The first term then leaves the pair in
    `memo` for its partner.  Otherwise each term makes its own."""
    if term in memo:
        return memo.pop(term)
    tr, other, z = term.tr, term.partner, draws.get(term.draws[0])
    share = False
    if other is not None:
        z_other = draws.get(other.draws[0])
        share = term.rows(z) == other.rows(z_other) and (z is None or z_other is None or z is z_other)
        if share and z is None:
            z = z_other
    if z is None:
        z = torch.randn(term.rows(None), tr.cfg.latent, device=tr.device)
    pair = tr._feature_pair(z, g_noise)
    if share:
        memo[other] = pair
    return pair


class CdcTerm(FeaturePairTerm):
    name, weights, batch, min_batch, draws = 'cdc', ('cdc_weight',), 'cdc_batch', 2, ('cdc_noise', 'cdc_layers')
    loss = staticmethod(cdc.distance_consistency_loss)


class DclGTerm(FeaturePairTerm):
    name, weights, batch, min_batch, draws = 'dcl_g', ('dcl_g_weight',), 'dcl_batch', 1, ('dcl_noise', 'dcl_layers')

    def loss(self, feats_t, feats_s, layers):       # the temperature is the trainer's to check: the D step's term reads it too
        return dcl.generator_contrastive_loss(feats_t, feats_s, layers, self.tr.cfg.dcl_tau)


class ClipTerm(GTerm):
    """'clip_dir' and / or 'clip_within' of one draw: z ~ N(0, I) [clip_batch, latent] through the frozen source generator (no
    grad) and through G with the same noise maps, both image batches through the encoder of the trainer's ClipGuide."""
    weights, draws = ('clip_dir_weight', 'clip_within_weight'), ('clip_noise',)

    def __init__(self, trainer):
        cfg = trainer.cfg
        if trainer.g_source is None or trainer.clip is None:
            raise ValueError('RickTrainer: clip_dir_weight / clip_within_weight > 0 need the frozen source generator and the '
                             'CLIP guide (g_source=, clip=ClipGuide(net, direction))')
        if cfg.clip_batch < (2 if cfg.clip_within_weight > 0 else 1):
            raise ValueError('RickTrainer: clip_batch must be >= 1, and >= 2 with clip_within_weight > 0')
        self.tr = trainer

    def __call__(self, draws, g_noise, memo):
        tr, cfg, z = self.tr, self.tr.cfg, draws.get('clip_noise')
        if z is None:
            z = torch.randn(cfg.clip_batch, cfg.latent, device=tr.device)
        if g_noise is None:
            g_noise = [n.expand(z.shape[0], -1, -1, -1).clone().normal_() for n in tr.g.make_noise()]
        with torch.no_grad():
            fake_s, _ = tr.g_source([z], noise=g_noise)
        fake_t, _ = tr.g([z], noise=g_noise)
        terms = tr.clip.terms(fake_t, fake_s, cfg.clip_dir_weight > 0, cfg.clip_within_weight > 0)
        return {name: (getattr(cfg, name + '_weight'), value) for name, value in terms.items()}


TERMS = (CdcTerm, DclGTerm, ClipTerm)                       # the order the terms are evaluated and added in
DRAWS = frozenset(k for cls in TERMS for k in cls.draws)    # every keyword g_step accepts beyond its own


def build(trainer):
    """Check the configuration against every term class, then make the terms that are on."""
    for cls in TERMS:
        cls.check(trainer.cfg)
    terms = [t for t in (cls.make(trainer) for cls in TERMS) if t is not None]
    pairs = [t for t in terms if isinstance(t, FeaturePairTerm)]
    if len(pairs) == 2:
        pairs[0].partner = pairs[1]
    return terms
