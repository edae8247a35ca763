"""RickTrainer._feature_pair: the one source / target forward pair behind the distance-consistency term, a method of its own
so that a further feature-pair term (rick_amd/gterms.py) can share it.  Stand-in generators (the generator itself has no CPU path),
built the way tests/test_cdc.py builds them."""
import torch

from rick_amd import cdc


def _nets(size=32):
    from rick_amd.models import Discriminator, Generator
    torch.manual_seed(0)
    g0 = Generator(size, 512, 2, channel_multiplier=1)

    def build():
        g, d = Generator(size, 512, 2, channel_multiplier=1), Discriminator(size, channel_multiplier=1)
        g.load_state_dict(g0.state_dict())
        return g, d
    return build


def _stand_in(gen, calls):
    ws = [p for n, p in gen.named_parameters() if n.startswith('convs.') and n.endswith('conv.weight')]

    def forward(styles, return_feats=False, noise=None, **kw):
        calls.append((torch.is_grad_enabled(), noise))
        z = styles[0]
        feats = [torch.tanh(z[:, k:k + 48].reshape(-1, 3, 4, 4) + (k + 1.0) * ws[k % len(ws)].flatten()[:48].view(1, 3, 4, 4)) + 1.0
                 for k in range(gen.n_latent - 1)]
        return None, feats
    return forward


def _trainer():
    from rick_amd.train import RickTrainer, TrainConfig
    build = _nets()
    g, d = build()
    g_ema, d_ema = build()
    src = build()[0]
    tr = RickTrainer(TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, cdc_weight=1000.0, cdc_batch=4), g, d, g_ema, d_ema,
                     g_source=src)
    with torch.no_grad():
        for p in tr.g.parameters():
            p.add_(0.05 * torch.randn(p.shape, generator=torch.Generator().manual_seed(p.numel())))
    t_calls, s_calls = [], []
    tr.g.forward, src.forward = _stand_in(tr.g, t_calls), _stand_in(src, s_calls)
    return tr, src, t_calls, s_calls


def test_feature_pair_runs_each_generator_once_and_the_source_without_grad():
    tr, src, t_calls, s_calls = _trainer()
    z = torch.randn(4, 512, generator=torch.Generator().manual_seed(2))
    maps = object()
    feats_t, feats_s = tr._feature_pair(z, maps)
    assert len(t_calls) == 1 and len(s_calls) == 1
    assert t_calls[0] == (True, maps) and s_calls[0] == (False, maps)          # the same noise maps; the source under no_grad
    assert len(feats_t) == len(feats_s) == tr.g.n_latent - 1
    assert all(f.requires_grad for f in feats_t) and not any(f.requires_grad for f in feats_s)


def test_cdc_term_is_the_loss_on_the_pair():
    tr, src, t_calls, s_calls = _trainer()
    z = torch.randn(4, 512, generator=torch.Generator().manual_seed(2))
    layers = [1, 3, 3, 5]
    (cdc_term,) = tr.g_terms                                                   # the only term that is on (rick_amd/gterms.py)
    weight, term = cdc_term({'cdc_noise': z, 'cdc_layers': layers}, None, {})['cdc']
    assert weight == 1000.0
    assert len(t_calls) == 1 and len(s_calls) == 1                             # one forward pair per term
    feats_t, feats_s = tr._feature_pair(z)
    assert torch.equal(term.detach(), cdc.distance_consistency_loss(feats_t, feats_s, layers).detach())
    assert float(term) > 0
