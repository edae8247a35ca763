"""CPU: DiffAugment's policy parsing, its host-side draws against the published composition, their ranges, the config field."""
import itertools

import numpy as np
import pytest
import torch

from tests import diffaug_f64 as O

SUBSETS = [','.join(c) for k in (1, 2, 3) for c in itertools.combinations(('color', 'translation', 'cutout'), k)]


def test_policy_parsing():
    from rick_amd.diffaug import parse_policy
    assert parse_policy('color,translation,cutout') == ('color', 'translation', 'cutout')
    assert [','.join(parse_policy(p)) for p in SUBSETS] == SUBSETS and len(SUBSETS) == 7
    for bad in ('', 'colour', 'cutout,color', 'color,color', 'color,', ',color', 'color, cutout', 'translation,color', None, 3):
        with pytest.raises(ValueError):
            parse_policy(bad)


@pytest.mark.parametrize('policy', SUBSETS)
@pytest.mark.parametrize('hw', [(8, 8), (9, 9), (12, 20)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_draws_and_closed_form_reproduce_the_published_composition(policy, hw):
    """One seed: the seven published steps in fp64 on the global RNG == the closed form on draw_params' records.  The composition
    casts the same fp32 draws, so the records carry no extra rounding: 1e-12 covers the fp64 arithmetic of either side."""
    from rick_amd.diffaug import apply_params, draw_params
    h, w = hw
    n = 4
    x = torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(7)) * 2 - 1
    for seed in range(6):
        torch.manual_seed(seed)
        want = O.compose(x.double(), policy)
        torch.manual_seed(seed)
        params = draw_params(n, h, w, policy)
        got = O.apply(x, params)
        assert float((got - want).abs().max()) <= 1e-12, (policy, hw, seed)
        # the library's own composed path (CPU tensors) on the same records
        assert float((apply_params(x.double(), params) - want).abs().max()) <= 1e-12
        # a private generator gives the same numbers as the global one
        again = draw_params(n, h, w, policy, generator=torch.Generator().manual_seed(seed))
        assert again.tobytes() == params.tobytes()


def test_left_out_stages_keep_their_identity_and_draw_nothing():
    from rick_amd.diffaug import draw_params, identity_params
    torch.manual_seed(3)
    p = draw_params(5, 9, 9, 'translation')
    q = identity_params(5)
    for k in ('b', 's', 'c', 'r0', 'r1', 'c0', 'c1'):
        assert np.array_equal(p[k], q[k])
    torch.manual_seed(3)
    sr = O.shift_range(9)
    assert np.array_equal(p['tr'], torch.randint(-sr, sr + 1, size=[5, 1, 1]).view(5).numpy())


@pytest.mark.parametrize('hw', [(8, 8), (9, 9), (12, 20)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_ranges_of_ten_thousand_draws(hw):
    from rick_amd.diffaug import check_params, draw_params
    h, w = hw
    p = draw_params(10_000, h, w, 'color,translation,cutout', generator=torch.Generator().manual_seed(11))
    assert p['b'].min() >= -0.5 and p['b'].max() <= 0.5
    assert p['s'].min() >= 0 and p['s'].max() <= 2
    assert p['c'].min() >= 0.5 and p['c'].max() <= 1.5
    sr, sc = O.shift_range(h), O.shift_range(w)
    assert sorted(set(p['tr'].tolist())) == list(range(-sr, sr + 1))
    assert sorted(set(p['tc'].tolist())) == list(range(-sc, sc + 1))
    assert (p['r0'] >= 0).all() and (p['r1'] <= h).all() and (p['r0'] < p['r1']).all()
    assert (p['c0'] >= 0).all() and (p['c1'] <= w).all() and (p['c0'] < p['c1']).all()
    assert (p['r1'] - p['r0']).max() == O.cut_size(h) and (p['c1'] - p['c0']).max() == O.cut_size(w)
    check_params(p, h, w)


def test_check_params_rejects_records_outside_the_image():
    from rick_amd.diffaug import check_params, identity_params
    for field, value in (('tr', 8), ('tr', -8), ('tc', 12), ('tc', -12), ('r0', -1), ('r1', 9), ('c0', -1), ('c1', 13), ('c', float('nan'))):
        p = identity_params(3)
        p[field][1] = value
        with pytest.raises(ValueError):
            check_params(p, 8, 12)
    check_params(identity_params(3), 8, 12)


def test_cpu_tensors_take_the_composed_path_with_gradients():
    from rick_amd.diffaug import diffaug
    x = (torch.rand(2, 3, 8, 8, generator=torch.Generator().manual_seed(1)) * 2 - 1).double().requires_grad_(True)
    y = diffaug(x, 'color,translation,cutout', generator=torch.Generator().manual_seed(5))
    torch.manual_seed(5)
    assert float((y.detach() - O.compose(x.detach(), 'color,translation,cutout')).abs().max()) <= 1e-12
    (g,) = torch.autograd.grad(y.sum(), x)
    assert g.shape == x.shape and float(g.abs().max()) > 0


def test_symbols_are_exported():
    import rick_amd.diffaug as DA
    for name in ('parse_policy', 'draw_params', 'DiffAugFn', 'DiffAugAdjFn', 'diffaug_fused', 'diffaug', 'PARAM_DTYPE'):
        assert name in DA.__all__ and hasattr(DA, name)
    assert DA.PARAM_DTYPE.itemsize == 40
    from rick_amd import _lib
    for name in ('rick_diffaug_workspace_bytes', 'rick_diffaug_fwd_f32', 'rick_diffaug_adj_f32', 'rick_diffaug_check_params'):
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.rick_diffaug_workspace_bytes(8, 256, 256) == 8 * 48 * 8


def test_config_default_and_the_trainer_refuses_both_augmentations():
    from rick_amd.train import RickTrainer, TrainConfig
    assert TrainConfig().diffaug == ''
    nets = [torch.nn.Linear(2, 2) for _ in range(4)]
    with pytest.raises(ValueError):
        RickTrainer(TrainConfig(size=32, batch=2, augment=True, diffaug='color'), *nets)
    with pytest.raises(ValueError):
        RickTrainer(TrainConfig(size=32, batch=2, diffaug='cutout,color'), *nets)
