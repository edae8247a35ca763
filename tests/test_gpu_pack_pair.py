"""The group pack of a network (rick_conv_pack_weights_multi) with PAIRED descriptors: a view and its transposed view of one
parameter are packed from one read of the source.  Both images must equal the single-weight kernel's (rick_conv_pack_weight
through `_pack(view, scale, None)`) byte for byte, trailer included — for whole and ragged tiles, strided views, either
registration order, unpaired views, and launches captured before a later view was registered."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SCALE = 0.37


def _net(shape, seed):
    from rick_amd.op import conv as cv
    torch.manual_seed(seed)
    mod = torch.nn.Linear(1, 1)                      # a module to hang the parameter on (PackGroup is per network)
    mod.w = torch.nn.Parameter(torch.randn(*shape, device=DEV))
    return cv, mod.w, cv.register_pack_group(mod)


def _update(cv, w):
    w.data.mul_(1.5).add_(0.01)
    cv.bump_weights_epoch([w])


def _check(cv, grp, w, views):
    """views: [(view, tag)].  After an update and one group refresh every image equals the single-weight pack of the
    updated values and differs from the image before the update."""
    before = [cv._pack(v, SCALE, (w, t)).clone() for v, t in views]
    _update(cv, w)
    assert grp.refresh()
    for (v, t), old in zip(views, before):
        multi = cv._pack(v, SCALE, (w, t))
        single = cv._pack(v, SCALE, None)
        assert multi.numel() == single.numel()
        assert torch.equal(multi, single), f'{t}: {int((multi != single).sum())} bytes differ'
        assert not torch.equal(multi, old)


CASES = [(32, 32, 3), (128, 256, 3), (130, 70, 3), (40, 24, 1), (64, 513, 3), (256, 128, 1)]


@pytest.mark.parametrize('O,I,k', CASES)
@pytest.mark.parametrize('order', ['view_first', 'transposed_first'])
def test_pair_equals_single_pack(O, I, k, order):
    cv, w, grp = _net((O, I, k, k), O + I + k)
    views = [(w, 'a/conv'), (w.transpose(0, 1), 'a/T/convT')]
    if order == 'transposed_first':
        views.reverse()
    _check(cv, grp, w, views)
    assert grp.n == 2 and grp.paired == 2 and grp.total_blocks == 0       # one pass over the source, no per-view blocks
    _check(cv, grp, w, views)                                              # and again on the steady-state table


@pytest.mark.parametrize('order', ['view_first', 'transposed_first'])
def test_pair_strided_view_of_larger_buffer(order):
    """The modulated convolutions pass weight[0] of a [1, Co, Ci, 3, 3] parameter; here additionally a window of a larger
    buffer: row stride above Ci * 9, a source offset that is no multiple of 16 bytes."""
    O, I = 70, 45
    cv, w, grp = _net((1, O + 3, I + 5, 3, 3), 7)
    view = w[0, 1:1 + O, 1:1 + I]              # 459 floats into the storage: 1836 bytes, 12 past a 16-byte boundary
    assert view.stride() == ((I + 5) * 9, 9, 3, 1) and view.data_ptr() % 16
    views = [(view, 'm/conv'), (view.transpose(0, 1), 'm/T/convT')]
    if order == 'transposed_first':
        views.reverse()
    _check(cv, grp, w, views)
    assert grp.paired == 2 and grp.total_blocks == 0


@pytest.mark.parametrize('O,I,k', [(130, 70, 3), (40, 24, 1)])
@pytest.mark.parametrize('which', ['view', 'transposed'])
def test_unpaired_view(O, I, k, which):
    cv, w, grp = _net((O, I, k, k), 3 * O + k)
    view = w if which == 'view' else w.transpose(0, 1)
    _check(cv, grp, w, [(view, 'a/conv')])
    assert grp.n == 1 and grp.paired == 0 and grp.total_blocks == cv.lib.rick_conv_pack_blocks(*view.shape[:2])


def test_unpaired_beside_pairs():
    """One table with a pair, a view on the per-view path between its two halves, and a 4 x 4 kernel (16 tap slices: above what
    the pair kernel stages, so the pair stays two per-view entries)."""
    from rick_amd.op import conv as cv
    torch.manual_seed(11)
    mod = torch.nn.Linear(1, 1)
    mod.a = torch.nn.Parameter(torch.randn(96, 40, 3, 3, device=DEV))
    mod.b = torch.nn.Parameter(torch.randn(33, 20, 1, 1, device=DEV))
    mod.c = torch.nn.Parameter(torch.randn(24, 36, 4, 4, device=DEV))
    grp = cv.register_pack_group(mod)
    views = [(mod.a, mod.a, 'a/conv'), (mod.b, mod.b, 'b/conv'), (mod.a, mod.a.transpose(0, 1), 'a/T/convT'),
             (mod.c, mod.c, 'c/conv'), (mod.c, mod.c.transpose(0, 1), 'c/T/convT')]
    before = [cv._pack(v, SCALE, (p, t)).clone() for p, v, t in views]
    for p in (mod.a, mod.b, mod.c):
        _update(cv, p)
    assert grp.refresh()
    assert grp.n == 5 and grp.paired == 2
    assert grp.total_blocks == sum(cv.lib.rick_conv_pack_blocks(o, i) for o, i in ((33, 20), (24, 36), (36, 24)))
    for (p, v, t), old in zip(views, before):
        multi = cv._pack(v, SCALE, (p, t))
        assert torch.equal(multi, cv._pack(v, SCALE, None)) and not torch.equal(multi, old), t


def test_one_buffer_per_distinct_view():
    """Requests are keyed by what determines the bytes, not by the caller's tag path."""
    cv, w, grp = _net((48, 40, 3, 3), 5)
    bufs = [cv._pack(w, SCALE, (w, tag)) for tag in ('a/conv', 'a/convT', 'a/T/T/conv')]
    bufs.append(cv._pack(w.transpose(0, 1).transpose(0, 1), SCALE, (w, 'a/T/T/conv')))
    assert len({b.data_ptr() for b in bufs}) == 1
    assert grp.n == 1 and len(grp.reqs) == 1
    other = cv._pack(w, 0.5, (w, 'a/conv'))                       # another scale is other bytes
    assert other.data_ptr() != bufs[0].data_ptr() and grp.n == 2
    _check(cv, grp, w, [(w, 'a/conv'), (w, 'a/T/T/conv')])


def test_captured_refresh_survives_later_registration():
    """A graph that holds refresh()'s launch bakes in the entry and block counts.  Views registered afterwards — the transposed
    view of an entry the graph packs on the per-view path among them — must not change what a replay writes for the views
    it knew."""
    from rick_amd.op import conv as cv
    torch.manual_seed(13)
    mod = torch.nn.Linear(1, 1)
    mod.a = torch.nn.Parameter(torch.randn(130, 70, 3, 3, device=DEV))
    mod.b = torch.nn.Parameter(torch.randn(64, 96, 3, 3, device=DEV))
    grp = cv.register_pack_group(mod)
    a, b = mod.a, mod.b
    known = [(a, a, 'a/conv'), (b, b, 'b/conv'), (b, b.transpose(0, 1), 'b/T/convT')]   # a: unpaired so far, b: a pair
    for p, v, t in known:
        cv._pack(v, SCALE, (p, t))
    for p in (a, b):
        _update(cv, p)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert grp.refresh()
    n_cap, blocks_cap = grp.n, grp.total_blocks
    assert n_cap == 3 and blocks_cap == cv.lib.rick_conv_pack_blocks(130, 70)
    graph.replay()
    for p, v, t in known:
        assert torch.equal(cv._pack(v, SCALE, (p, t)), cv._pack(v, SCALE, None)), t

    later = [(a, a.transpose(0, 1), 'a/T/convT')]                # pairs with entry 0, which the captured launch packs by itself
    for p, v, t in later:
        cv._pack(v, SCALE, (p, t))
    assert grp.n == 4 and grp.paired == 4
    assert int(grp.host['blk_begin'][0]) == 0 and grp.total_blocks == blocks_cap      # entry 0 keeps the blocks the graph runs
    for p in (a, b):
        p.data.mul_(0.5).sub_(0.02)
    stale = [cv._pack(v, SCALE, None) for p, v, t in known]      # (single packs of the NEW values)
    graph.replay()                                               # no epoch bump: only the replay has repacked
    torch.cuda.synchronize()
    for (p, v, t), ref in zip(known, stale):
        assert torch.equal(grp.reqs[(v.data_ptr(), tuple(v.shape), v.stride(), SCALE)]['buf'], ref), t
    # and the eager launch over the grown table packs all four
    for p in (a, b):
        _update(cv, p)
    assert grp.refresh()
    for p, v, t in known + later:
        assert torch.equal(cv._pack(v, SCALE, (p, t)), cv._pack(v, SCALE, None)), t
