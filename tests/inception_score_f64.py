"""fp64 restatement of the reference's Inception Score (gan_training/metrics/inception_score.py:12-58): torchvision's
Inception3 in eval mode without its input transform, on the images as they are or after nn.Upsample(size=(299, 299),
mode='bilinear'), fc, softmax, and exp of the mean KL divergence to the split's marginal with scipy.stats.entropy's
renormalisation of both arguments, written by hand (scipy is not needed).

tests.inception_f64.forward_f64 always resizes to 299 and applies the FID wrapper's affine, so the blocks are restated here
from its layer table (BatchNorm not folded) for an input that is used as it is.

with_head(sd, images, size): torchvision's synthetic fc.weight * 0.01 with a zero bias gives a near-uniform softmax and a score
of about 1, whatever the network computes.  The head drawn here makes the score mean something: a seeded normal fc.weight,
scaled so that the fp64 logits of `images` spread with a standard deviation of 3 around their per-class mean over the images,
and a bias that removes most of that per-class mean (the pool3 features of a synthetic network share a large common part,
which alone would give every image the same softmax).  The fp64 score of the set is asserted to lie above 1.5."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.inception_f64 import UNIT, synthetic_state_dict

CLASSES, POOL3 = 1000, 2048


def pool3_f64(sd, x):
    """torchvision Inception3 from Conv2d_1a_3x3 to the global average pool on x [N, 3, H, W] as given, in fp64."""
    def bc(name, v):
        u = UNIT[name]
        y = F.conv2d(v, sd[f'{name}.conv.weight'].double(), None, u['s'], u['p'])
        y = F.batch_norm(y, sd[f'{name}.bn.running_mean'].double(), sd[f'{name}.bn.running_var'].double(),
                         sd[f'{name}.bn.weight'].double(), sd[f'{name}.bn.bias'].double(), False, 0.0, 1e-3)
        return F.relu(y)

    def chain(prefix, names, v):
        for n in names:
            v = bc(f'{prefix}.{n}', v)
        return v

    def avg(v):
        return F.avg_pool2d(v, 3, 1, 1, count_include_pad=True)

    x = x.double()
    x = F.max_pool2d(bc('Conv2d_2b_3x3', bc('Conv2d_2a_3x3', bc('Conv2d_1a_3x3', x))), 3, 2)
    x = F.max_pool2d(bc('Conv2d_4a_3x3', bc('Conv2d_3b_1x1', x)), 3, 2)
    for m in ('Mixed_5b', 'Mixed_5c', 'Mixed_5d'):
        x = torch.cat([bc(f'{m}.branch1x1', x), chain(m, ['branch5x5_1', 'branch5x5_2'], x),
                       chain(m, ['branch3x3dbl_1', 'branch3x3dbl_2', 'branch3x3dbl_3'], x), bc(f'{m}.branch_pool', avg(x))], 1)
    m = 'Mixed_6a'
    x = torch.cat([bc(f'{m}.branch3x3', x), chain(m, ['branch3x3dbl_1', 'branch3x3dbl_2', 'branch3x3dbl_3'], x),
                   F.max_pool2d(x, 3, 2)], 1)
    for m in ('Mixed_6b', 'Mixed_6c', 'Mixed_6d', 'Mixed_6e'):
        x = torch.cat([bc(f'{m}.branch1x1', x), chain(m, ['branch7x7_1', 'branch7x7_2', 'branch7x7_3'], x),
                       chain(m, [f'branch7x7dbl_{i}' for i in range(1, 6)], x), bc(f'{m}.branch_pool', avg(x))], 1)
    m = 'Mixed_7a'
    x = torch.cat([chain(m, ['branch3x3_1', 'branch3x3_2'], x), chain(m, [f'branch7x7x3_{i}' for i in range(1, 5)], x),
                   F.max_pool2d(x, 3, 2)], 1)
    for m in ('Mixed_7b', 'Mixed_7c'):
        t3 = bc(f'{m}.branch3x3_1', x)
        td = chain(m, ['branch3x3dbl_1', 'branch3x3dbl_2'], x)
        x = torch.cat([bc(f'{m}.branch1x1', x), bc(f'{m}.branch3x3_2a', t3), bc(f'{m}.branch3x3_2b', t3),
                       bc(f'{m}.branch3x3dbl_3a', td), bc(f'{m}.branch3x3dbl_3b', td), bc(f'{m}.branch_pool', avg(x))], 1)
    return x.mean((2, 3))


def features_f64(sd, images, size):
    """size=None: the reference's resize=True (bilinear to 299, align_corners=False); size=(H, W): the images as they are."""
    x = images.double()
    if size is None:
        x = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False)
    else:
        assert tuple(x.shape[2:]) == tuple(size)
    with torch.no_grad():
        return pool3_f64(sd, x)


def logits_f64(sd, images, size, feats=None):
    f = features_f64(sd, images, size) if feats is None else feats
    return f @ sd['fc.weight'].double().t() + sd['fc.bias'].double()


def softmax_f64_of_f32(logits):
    """The reference's preds: F.softmax of the fp32 logits in fp32, stored as float64."""
    return torch.softmax(torch.as_tensor(logits).float(), dim=-1).double().numpy()


def entropy_f64(pk, qk):
    """scipy.stats.entropy(pk, qk): both renormalised to sum 1, sum pk log(pk / qk), terms with pk == 0 are 0."""
    pk, qk = np.asarray(pk, np.float64), np.asarray(qk, np.float64)
    pk, qk = pk / pk.sum(), qk / qk.sum()
    nz = pk > 0
    return float(np.sum(pk[nz] * np.log(pk[nz] / qk[nz])))


def score_from_preds(preds, splits=1):
    """inception_score.py:46-58 on preds [N, C] float64 -> (mean, std) floats."""
    preds = np.asarray(preds, np.float64)
    n = preds.shape[0]
    out = []
    for k in range(splits):
        part = preds[k * (n // splits):(k + 1) * (n // splits)]
        py = part.mean(0)
        out.append(np.exp(np.mean([entropy_f64(part[i], py) for i in range(part.shape[0])])))
    return float(np.mean(out)), float(np.std(out))


def score_f64(logits, splits=1):
    """The score of exact logits, all in fp64 (softmax included): what the network's fp32 arithmetic is measured against."""
    return score_from_preds(torch.softmax(torch.as_tensor(logits).double(), dim=-1).numpy(), splits)


_HEADS = {}


def with_head(images, size, seed=0, key=None):
    """-> (sd with a head fitted to `images`, fp64 logits [N, 1000] of `images`); cached under `key`."""
    if key is not None and key in _HEADS:
        sd, ref = _HEADS[key]
        return dict(sd), ref
    sd = synthetic_state_dict(0)
    f = features_f64(sd, images, size)
    g = torch.Generator().manual_seed(77 + seed)
    w = torch.randn(CLASSES, POOL3, generator=g, dtype=torch.float64)
    z = (f - f.mean(0)) @ w.t()                               # what differs between the images
    w = w * (3.0 / float(z.std()))
    sd['fc.weight'] = w.float()
    sd['fc.bias'] = (-(sd['fc.weight'].double() @ f.mean(0)) + 0.5 * torch.randn(CLASSES, generator=g, dtype=torch.float64)).float()
    ref = logits_f64(sd, images, size, feats=f)
    spread = float((ref - ref.mean(0)).std())
    assert 2.5 < spread < 3.5, spread
    assert score_f64(ref)[0] > 1.5, score_f64(ref)
    if key is not None:
        _HEADS[key] = (dict(sd), ref)
    return sd, ref


def smooth_images(n, h, w, seed):
    """Seeded images in [-1, 1] with structure at several scales (a bilinear resize of pure noise would lose most of it)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(n, 3, h, w)
    for low in (4, 11, max(h, w)):
        x = x + F.interpolate(torch.rand(n, 3, low, low, generator=g) * 2 - 1, size=(h, w), mode='bilinear', align_corners=False)
    return (x / 3 * 1.5).clamp_(-1, 1).contiguous()
