"""Plain fp64 restatement of the cross-domain distance-consistency loss, the way it is customarily written: the literal double
loop over (i, j != i) with F.cosine_similarity on flattened rows, nn.Softmax(dim=1), nn.KLDivLoss() on log(softmax).  Nothing
is imported from rick_amd.cdc."""
import torch
import torch.nn.functional as F


def pairwise_cosine_f64(feats, layers):
    """feats: list of [B, ...] tensors; layers: B indices -> [B, B - 1] fp64 (autograd flows into fp64 feats)."""
    B = len(layers)
    rows = []
    for i in range(B):
        f = feats[int(layers[i])].double()
        row = []
        for j in range(B):
            if j == i:
                continue
            row.append(F.cosine_similarity(f[i].reshape(1, -1), f[j].reshape(1, -1)))
        rows.append(torch.cat(row))
    return torch.stack(rows)


def loss_f64(feats_target, feats_source, layers):
    sfm = torch.nn.Softmax(dim=1)
    kl = torch.nn.KLDivLoss()
    with torch.no_grad():
        ps = sfm(pairwise_cosine_f64(feats_source, layers))
    pt = sfm(pairwise_cosine_f64(feats_target, layers))
    return kl(torch.log(pt), ps)


def random_feats(shapes, B, seed, offset=1.0):
    """fp32 feature lists of a source and a target generator: N(0, 1) plus a common offset (cosines near 1, as behind a
    LeakyReLU); the target is a perturbed source."""
    g = torch.Generator().manual_seed(seed)
    src = [torch.randn(B, *s, generator=g) + offset for s in shapes]
    tgt = [f + 0.5 * torch.randn(B, *s, generator=g) for f, s in zip(src, shapes)]
    return tgt, src
