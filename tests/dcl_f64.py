"""Plain fp64 restatement of DCL's two contrastive losses, written literally: a double loop, F.cosine_similarity on flattened
rows, log_softmax.  Nothing is imported from rick_amd.dcl."""
import torch
import torch.nn.functional as F


def _cos(u, v):
    return F.cosine_similarity(u.reshape(1, -1), v.reshape(1, -1))[0]


def cl1_f64(feats_t, feats_s, layers, tau=0.07):
    """mean_i -log softmax_j(cos(t_i, s_j) / tau)[i] at layer l_i; autograd flows into fp64 feats_t."""
    B = len(layers)
    terms = []
    for i in range(B):
        ft, fs = feats_t[int(layers[i])].double(), feats_s[int(layers[i])].double().detach()
        logits = torch.stack([_cos(ft[i], fs[j]) / tau for j in range(B)])
        terms.append(-torch.log_softmax(logits, 0)[i])
    return torch.stack(terms).mean()


def cl2_f64(feats_fake_t, feats_fake_s, feats_real_t, layers, tau=0.07):
    """mean_i -log softmax([cos(a_i, p_i), cos(a_i, x_1), ..., cos(a_i, x_M)] / tau)[0] at layer l_i; autograd flows into fp64
    anchors and negatives."""
    B = len(layers)
    terms = []
    for i in range(B):
        l = int(layers[i])
        a, p, x = feats_fake_t[l].double(), feats_fake_s[l].double().detach(), feats_real_t[l].double()
        logits = [_cos(a[i], p[i]) / tau]
        for j in range(x.shape[0]):
            logits.append(_cos(a[i], x[j]) / tau)
        terms.append(-torch.log_softmax(torch.stack(logits), 0)[0])
    return torch.stack(terms).mean()


def random_feats(shapes, B, seed, offset=1.0, perturb=0.5):
    """An fp32 feature list: N(0, 1) plus a common offset (cosines near 1, as behind a LeakyReLU)."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, *s, generator=g) * perturb + offset + torch.randn(1, *s, generator=g) for s in shapes]
