"""CLIP-guided adaptation losses on the image tower of rick_amd/clip.py: the directional loss of StyleGAN-NADA (Gal et al.,
2021) and the in-domain consistency loss of Mind-the-Gap (Zhu et al., 2022), as terms of the generator step.  Formulas as
recalled, unverified against the papers' code.

    net = ClipImageFeatures.load(src, batch=25).prepare_grad(grad_batch=4)
    guide = ClipGuide(net, domain_direction(net, source_images, target_images))
    trainer = RickTrainer(TrainConfig(clip_dir_weight=1.0, clip_within_weight=0.5, clip_batch=4), ..., g_source=g_src, clip=guide)

    e_s, e_t = net(g_source(z)), net.encode(g(z))        # the frozen generator's embeddings need no gradient
    loss = directional_loss(e_t, e_s, direction) + within_loss(e_t, e_s)

The heads act on [N, D] embeddings: a few thousand numbers, plain fp32 torch compositions on the embeddings' device.  The hot
path is ``ClipImageFeatures.encode``'s backward pass (HIP kernels, include/rick_hip.h "CLIP").  Wherever a direction is
expected, any [D] vector is accepted: ``domain_direction`` derives one from two image sets, ``text_direction`` from two
prompts through the text tower (rick_amd/cliptext.py, rick_amd/cliptok.py).

    direction = text_direction(ClipTextFeatures.load(src), ClipTokenizer.load(vocab_json, merges_txt), 'photo', 'sketch')

With n(e) = e / |e| and cos = F.cosine_similarity (eps 1e-8):

* domain_direction = n(mean_i n(e(target_i)) - mean_i n(e(source_i)));
* text_direction = n(mean_t n(E(template_t(target))) - mean_t n(E(template_t(source)))), E the text tower;
* directional_loss = mean_i (1 - cos(n(e_t,i) - n(e_s,i), direction));
* within_loss = mean over pairs i < j of 1 - cos(n(e_s,i) - n(e_s,j), n(e_t,i) - n(e_t,j)).
"""
import torch
import torch.nn.functional as F

WHO = 'clipguide'


def _pair(e_t, e_s):
    if e_t.dim() != 2 or e_t.shape != e_s.shape:
        raise ValueError(f'{WHO}: expected embeddings [N, D] of one shape, got {tuple(e_t.shape)} and {tuple(e_s.shape)}')
    return F.normalize(e_t.float(), dim=1, eps=0), F.normalize(e_s.float(), dim=1, eps=0)


@torch.no_grad()
def domain_direction(net, source_images, target_images):
    """[D] fp32 unit vector from the source set's mean normalised embedding to the target set's; no gradient."""
    means = [F.normalize(net(x).float(), dim=1, eps=0).mean(0) for x in (source_images, target_images)]
    return F.normalize(means[1] - means[0], dim=0, eps=0)


@torch.no_grad()
def text_direction(tnet, tok, source, target, templates=('a photo of a {}.',)):
    """[D] fp32 unit vector from the source word's mean normalised text embedding over the templates to the target word's, on
    the text tower's device; no gradient.  tnet: ClipTextFeatures, tok: ClipTokenizer (any callable from a list of strings to
    id rows)."""
    if not templates:
        raise ValueError(f'{WHO}: text_direction needs at least one template')
    means = []
    for word in (source, target):
        ids = tok([t.format(word) for t in templates])
        means.append(F.normalize(tnet(ids.to(tnet.device)).float(), dim=1, eps=0).mean(0))
    direction = F.normalize(means[1] - means[0], dim=0, eps=0)
    if not torch.isfinite(direction).all():
        raise ValueError(f'{WHO}: the embeddings of {source!r} and {target!r} coincide: no direction between them')
    return direction


def directional_loss(e_t, e_s, direction):
    """StyleGAN-NADA's loss: mean_i (1 - cos(n(e_t,i) - n(e_s,i), direction)); direction: any [D] vector."""
    t, s = _pair(e_t, e_s)
    if direction.dim() != 1 or direction.shape[0] != t.shape[1]:
        raise ValueError(f'{WHO}: expected a direction [{t.shape[1]}], got {tuple(direction.shape)}')
    return (1 - F.cosine_similarity(t - s, direction.float()[None], dim=1, eps=1e-8)).mean()


def within_loss(e_t, e_s):
    """Mind-the-Gap's in-domain consistency: the differences between the batch members' embeddings keep their directions,
    mean over pairs i < j of 1 - cos(n(e_s,i) - n(e_s,j), n(e_t,i) - n(e_t,j)).  N >= 2."""
    t, s = _pair(e_t, e_s)
    if t.shape[0] < 2:
        raise ValueError(f'{WHO}: within_loss needs at least 2 embeddings, got {t.shape[0]}')
    i, j = torch.triu_indices(t.shape[0], t.shape[0], 1, device=t.device)
    return (1 - F.cosine_similarity(s[i] - s[j], t[i] - t[j], dim=1, eps=1e-8)).mean()


class ClipGuide:
    """The encoder and the direction of the trainer's CLIP terms (RickTrainer(..., clip=ClipGuide(net, direction)))."""

    def __init__(self, net, direction):
        direction = torch.as_tensor(direction)
        if direction.dim() != 1 or direction.shape[0] != net.cfg.dim or not torch.isfinite(direction).all():
            raise ValueError(f'ClipGuide: expected a finite direction [{net.cfg.dim}], got {tuple(direction.shape)}')
        self.net, self.direction = net, direction.detach().to(net.device, torch.float32)

    def terms(self, fake_t, fake_s, directional=True, within=True):
        """The unweighted terms of target images (with gradient) against source images (without), {'clip_dir', 'clip_within'}."""
        with torch.no_grad():
            e_s = self.net(fake_s)
        e_t = self.net.encode(fake_t)
        out = {}
        if directional:
            out['clip_dir'] = directional_loss(e_t, e_s, self.direction)
        if within:
            out['clip_within'] = within_loss(e_t, e_s)
        return out
