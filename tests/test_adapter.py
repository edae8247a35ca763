"""rick_amd.adapter on the CPU: the state_dict / load_state_dict rule of FlatAdapter on a toy subclass (validate everything, then
copy in place), the message prefix of the two real adapters, and KmlState.set_rows_from_index_sets.  CPU-only: no launch."""
import pytest
import torch
from torch import nn

from tests.test_kml import SHAPES


def _flat(seed=0):
    from rick_amd.flat import FlatParams
    g = torch.Generator().manual_seed(seed)
    named = [(n, nn.Parameter(torch.randn(*s, generator=g))) for n, s in SHAPES]
    return FlatParams(named, lambda n: 'convs' in n)


def _toy(seed=0):
    """One fp32 factor g[co] per layer; nothing but what the base asks of a subclass for persistence."""
    from rick_amd.adapter import FlatAdapter

    class Toy(FlatAdapter):
        def __init__(self, flat):
            super().__init__(flat, None, 'toy', lambda p: p.dim() >= 4)
            self.w0 = flat.flat[self.lo:self.hi].detach().clone()
            self._own_factors([(f'g.{n}', nn.Parameter(torch.zeros(self.shape3[n][0]))) for n in self.names], 0.01, (0.0, 0.99))
            self.loaded = []

        def _entries(self):
            out = []
            for n in self.names:
                a, b = self.segment(n)
                lo, hi, shape = self.fac_range(f'g.{n}')
                out += [(f'w0.{n}', tuple(self.flat.params[self.flat.index[n]].shape), torch.float32, self.w0[a:b]),
                        (f'g.{n}', shape, torch.float32, self.fac.flat[lo:hi]), (f'm.g.{n}', shape, torch.float32, self.optim.m[lo:hi]),
                        (f'v.g.{n}', shape, torch.float32, self.optim.v[lo:hi])]
            return out

        def _loaded(self, extra):
            self.loaded.append(extra)

    return Toy(_flat(seed))


def _randomise(t, seed):
    g = torch.Generator().manual_seed(seed)
    cover = torch.zeros(t.fac.total)                           # the factors' own elements (the padding stays zero)
    for o, size in zip(t.fac.offsets, t.fac.sizes):
        cover[int(o):int(o) + size] = 1
    with torch.no_grad():
        for buf in (t.fac.flat, t.optim.m, t.optim.v):
            buf.copy_(torch.rand(buf.shape, generator=g) * cover)
    t.optim.steps[:] = [seed + i for i in range(len(t.optim.steps))]
    t.optim.sync_steps_to_device()


def _live(t):
    return t.w0, t.fac.flat, t.optim.m, t.optim.v, t.optim.steps_dev


def test_base_class_state_dict_and_load_rule():
    a = _toy()
    assert a.names == ['convs.0.w', 'convs.1.w', 'convs.2.skip'] and a.owned == [n for n, _ in SHAPES if 'convs' in n]
    assert a.fac_range('g.convs.1.w') == (64, 64 + 7, (7,))
    _randomise(a, 3)
    sd = a.state_dict()
    assert set(sd) == {'steps'} | {key for key, _, _, _ in a._entries()}
    assert all(sd[key].shape == shape and sd[key].dtype == dtype for key, shape, dtype, _ in a._entries())
    assert sd['steps'].dtype == torch.int64 and sd['steps'].tolist() == [3, 4, 5]
    assert all(sd[key].data_ptr() != dst.data_ptr() for key, _, _, dst in a._entries())      # copies
    b = _toy(seed=1)
    _randomise(b, 7)
    ptrs = [x.data_ptr() for x in _live(b)] + [p.data_ptr() for p in b.fac.params]
    params = b.flat.flat.clone()
    b.load_state_dict(sd)
    assert ptrs == [x.data_ptr() for x in _live(b)] + [p.data_ptr() for p in b.fac.params]
    assert torch.equal(b.flat.flat, params)                    # the parameters are not written
    assert all(torch.equal(a.snapshot(n), b.snapshot(n)) for n in a.names)     # (w0 elsewhere in the slice is not part of the state)
    assert all(torch.equal(x, y) for x, y in zip(_live(a)[1:], _live(b)[1:])) and b.optim.steps == [3, 4, 5] and b.loaded == [{}]
    sd2 = b.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    # one bad entry among good ones that differ from what is live: the key is named, nothing live is touched
    snap = [x.clone() for x in _live(b)]
    nan = torch.zeros(9)
    nan[4] = float('nan')
    for key, bad, exc in (('v.g.convs.2.skip', torch.zeros(8), ValueError), ('w0.convs.1.w', torch.zeros(7, 4, 3, 3), ValueError),
                          ('m.g.convs.0.w', torch.zeros(6, dtype=torch.float64), ValueError), ('g.convs.2.skip', nan, ValueError),
                          ('v.g.convs.2.skip', None, KeyError), ('steps', None, KeyError),
                          ('steps', torch.zeros(2, dtype=torch.int64), ValueError), ('steps', torch.zeros(3, dtype=torch.int32), ValueError),
                          ('steps', torch.tensor([1, -1, 2]), ValueError)):
        broken = {k: v + 1 for k, v in sd.items()}
        if bad is None:
            del broken[key]
        else:
            broken[key] = bad
        with pytest.raises(exc, match='toy: .*' + key.replace('.', r'\.')):
            b.load_state_dict(broken)
        assert all(torch.equal(x, y) for x, y in zip(_live(b), snap)) and b.optim.steps == [3, 4, 5] and len(b.loaded) == 1
    b.load_state_dict({k: v + 1 for k, v in sd.items()})       # and the good ones alone do load
    assert torch.equal(b.optim.m[:6], a.optim.m[:6] + 1) and b.optim.steps == [4, 5, 6] and b.optim.steps_dev.tolist() == [4, 5, 6]


def test_error_prefixes():
    """Every message of an adapter carries its own tag and never the other module's."""
    from rick_amd.kml import KmlState
    from rick_amd.svd import SvdAdapter
    flat = _flat()
    for make, tag, other in ((lambda names: KmlState(flat, 2, names=names), 'kml', 'svd'),
                             (lambda names: SvdAdapter(flat, names=names), 'svd', 'kml')):
        for names, exc, what in ((['nope'], KeyError, 'nope'), (['head.w'], ValueError, 'outside the optimised slice'),
                                 (['convs.0.w', 'convs.0.w'], ValueError, 'twice'), ([], ValueError, 'no parameter'),
                                 (['convs.0.b'], ValueError, 'two dims')):
            with pytest.raises(exc) as e:
                make(names)
            msg = e.value.args[0]
            assert msg.startswith(f'{tag}: ') and what in msg and other not in msg, (tag, names, msg)


def test_set_rows_from_index_sets():
    from rick_amd.kml import KmlState
    k = KmlState(_flat(), 2, generator=torch.Generator().manual_seed(5))
    n = 'convs.0.w'                                            # 6 rows
    k.set_rows_from_index_sets({n: [0, 2, 5]}, {n: [2]})       # frozen and not pruned
    assert k.rows[n].tolist() == [True, False, False, False, False, True] and k.flagged == 2
    assert not k.rows['convs.1.w'].any() and not k.rows['convs.2.skip'].any()      # in neither set: nothing is flagged
    assert torch.equal(k.snapshot(n)[0], k.weight(n)[0]) and not k.snapshot(n)[2].any()
    k.set_rows_from_index_sets({n: [0, 2, 5]}, None)
    assert k.rows[n].tolist() == [True, False, True, False, False, True] and k.flagged == 3
    k.set_rows_from_index_sets(None, {n: [2]})
    assert k.flagged == 0
    k.set_rows_from_index_sets(None, None)
    assert k.flagged == 0 and k.nblocks == 0
