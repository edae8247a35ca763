"""CPU: the InceptionV3 feature extractor (rick_amd/inception.py) — loader, layer table, and the CPU composition against the
independent fp64 restatement (tests/inception_f64.py)."""
import pytest
import torch

from rick_amd.inception import InceptionV3Features, expected_keys, fold, units
from tests.inception_f64 import TABLE, forward_f64, synthetic_state_dict, table_keys, wrapper_layout


def test_layer_table_has_94_units_and_the_tables_keys():
    assert len(units()) == 94 == len(TABLE)
    assert expected_keys() == table_keys()
    assert len(expected_keys()) == 94 * 5
    ours = {u[0]: (u[1], u[2], u[3], u[4], u[5]) for u in units()}
    theirs = {u['name']: (u['ci'], u['co'], u['k'], u['s'], u['p']) for u in TABLE}
    assert ours == theirs


def test_loader_accepts_both_layouts_with_identical_folding():
    sd = synthetic_state_dict(0)
    a = fold(sd)
    b = fold(wrapper_layout(sd))
    assert a.keys() == b.keys() and len(a) == 94
    for k in a:
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]), k
    # the fold itself, spot-checked in fp64
    n = 'Mixed_6c.branch7x7dbl_3'
    s = sd[f'{n}.bn.weight'].double() / (sd[f'{n}.bn.running_var'].double() + 1e-3).sqrt()
    torch.testing.assert_close(a[n][0].double(), sd[f'{n}.conv.weight'].double() * s[:, None, None, None], rtol=1e-7, atol=0)
    torch.testing.assert_close(a[n][1].double(), sd[f'{n}.bn.bias'].double() - sd[f'{n}.bn.running_mean'].double() * s,
                               rtol=1e-6, atol=1e-7)


def test_loader_reads_a_file(tmp_path):
    sd = synthetic_state_dict(0)
    p = tmp_path / 'inception.pt'
    torch.save(sd, p)
    net = InceptionV3Features.load(str(p), device='cpu', dims=64)
    assert torch.equal(net.folded['Conv2d_1a_3x3'][0], fold(sd)['Conv2d_1a_3x3'][0])


def test_loader_rejects_missing_and_misshaped_keys():
    sd = synthetic_state_dict(0)
    bad = dict(sd)
    del bad['Mixed_6b.branch7x7_2.bn.running_var']
    with pytest.raises(KeyError, match='Mixed_6b.branch7x7_2.bn.running_var'):
        InceptionV3Features.load(bad, device='cpu')
    bad = dict(sd)
    bad['Mixed_7c.branch3x3dbl_3b.conv.weight'] = torch.zeros(384, 384, 1, 3)
    with pytest.raises(ValueError, match='Mixed_7c.branch3x3dbl_3b.conv.weight'):
        InceptionV3Features.load(bad, device='cpu')
    bad = wrapper_layout(sd)
    del bad['blocks.2.3.branch3x3.conv.weight']
    with pytest.raises(KeyError, match='Mixed_6a.branch3x3.conv.weight'):
        InceptionV3Features.load(bad, device='cpu')


def test_extractor_refuses_other_dtypes():
    net = InceptionV3Features.load(synthetic_state_dict(0), device='cpu', dims=64)
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 32, 32, dtype=torch.float64))
    with pytest.raises(ValueError):
        InceptionV3Features.load(synthetic_state_dict(0), device='cpu', dims=100)


@pytest.mark.parametrize('dims', [64, 192, 768, 2048])
def test_cpu_path_matches_fp64_restatement(dims):
    sd = synthetic_state_dict(0)
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(7)) * 2 - 1
    ref = forward_f64(sd, x, dims)
    net = InceptionV3Features.load(sd, device='cpu', dims=dims)
    got = net(x)
    assert got.shape == (2, dims) and got.dtype == torch.float32
    err = float((got.double() - ref).abs().max() / ref.abs().max())
    print(f'dims {dims}: max |d| / max |f64| = {err:.3e}')
    assert err <= 1e-4, err
    assert float(ref.abs().max()) > 0.05            # the calibrated weights keep activations O(1) to the end


@pytest.mark.parametrize('hw', [(128, 128), (256, 256), (300, 280)])
def test_resize_matches_interpolate_fp64(hw):
    """The CPU composition's first stage (resize + affine) against F.interpolate in fp64, through the dims=64 stem."""
    from rick_amd.inception import MEAN, STD
    x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(3)) * 2 - 1
    sd = synthetic_state_dict(0)
    net = InceptionV3Features.load(sd, device='cpu', dims=64)
    ref = forward_f64(sd, x, 64)
    err = float((net(x).double() - ref).abs().max() / ref.abs().max())
    assert err <= 1e-4, err
    assert len(MEAN) == len(STD) == 3
