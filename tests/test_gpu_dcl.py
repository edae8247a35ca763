"""rick_xgram_f32 / rick_xrowmix_f32 and the dual contrastive losses on them (rick_amd/dcl.py, rick_amd/csrc/gram.hip) against
fp64.

Every bound follows the fourfold rule of tests/test_gpu_cdc.py: four times the error that the plain fp32 torch composition of the
same quantity makes against the same fp64 reference on the same inputs, measured here per case (never a constant).  The figures
each test prints (run with -s) are the ones quoted in DESIGN.md."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (Ba, Bb, n): one element; below a float4; a partial block; two slices, unaligned; two full slices at the register maximum;
# 17 slices; past 4096 * 1024 elements, where the slices grow to 8192 (scalar and 16-byte loads)
SHAPES = [(1, 1, 1), (2, 3, 3), (3, 1, 255), (4, 4, 4097), (8, 8, 8192), (5, 2, 67015), (2, 2, 4096 * 1024 + 4101),
          (2, 2, 4096 * 1024 + 4104)]
# 'mixed': a starts one float into its buffer, b is 16-byte aligned, n % 4 == 0 (two slices);  'channels_last': 4-D operands in
# the generator's layout;  'halves': a = f[:4], b = f[4:] of one channels-last tensor
CASES = SHAPES + ['mixed', 'channels_last', 'halves']
_cache = {}


def _ids(s):
    return s if isinstance(s, str) else 'x'.join(str(v) for v in s)


def _case(case):
    """(a, b) fp32 on the CPU as the device will see them (N(0, 1) + 1: cosines near 1, as behind a LeakyReLU), their rows in
    memory order, and the fp64 products C, na, nb — computed once per case and shared."""
    if case not in _cache:
        g = torch.Generator().manual_seed(77 if isinstance(case, str) else sum(case))
        if case == 'channels_last':
            a = (torch.randn(3, 24, 9, 7, generator=g) + 1.0).contiguous(memory_format=torch.channels_last)
            b = (torch.randn(2, 24, 9, 7, generator=g) + 1.0).contiguous(memory_format=torch.channels_last)
            ra, rb = a.permute(0, 2, 3, 1).reshape(3, -1), b.permute(0, 2, 3, 1).reshape(2, -1)
        elif case == 'halves':
            f = (torch.randn(8, 6, 5, 7, generator=g) + 1.0).contiguous(memory_format=torch.channels_last)
            a, b = f[:4], f[4:]
            ra, rb = a.permute(0, 2, 3, 1).reshape(4, -1), b.permute(0, 2, 3, 1).reshape(4, -1)
        else:
            Ba, Bb, n = (3, 2, 4104) if case == 'mixed' else case
            a, b = torch.randn(Ba, n, generator=g) + 1.0, torch.randn(Bb, n, generator=g) + 1.0
            ra, rb = a, b
        a64, b64 = ra.double(), rb.double()
        _cache[case] = (a, b, ra, rb, (a64 @ b64.t(), (a64 * a64).sum(1), (b64 * b64).sum(1)))
    return _cache[case]


def _to_dev(case):
    a, b = _case(case)[:2]
    if case == 'mixed':
        buf = torch.empty(a.numel() + 1, device=DEV)
        ad = buf[1:].view(a.shape)
        ad.copy_(a)
        bd = b.to(DEV)
        assert ad.data_ptr() % 16 == 4 and bd.data_ptr() % 16 == 0 and a.shape[1] % 4 == 0
        return ad, bd
    if case == 'halves':
        f = torch.cat([a, b]).contiguous(memory_format=torch.channels_last).to(DEV)
        return f[:4], f[4:]
    return a.to(DEV), b.to(DEV)


def _xgram_err(got, ref):
    """The largest error of C, na, nb, each relative to the product of its two rows' norms."""
    C, na, nb = (t.double().cpu() for t in got)
    rC, ra, rb = ref
    da, db = ra.sqrt(), rb.sqrt()
    return max(float(((C - rC).abs() / (da[:, None] * db[None, :])).max()), float(((na - ra).abs() / ra).max()),
               float(((nb - rb).abs() / rb).max()))


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_xgram_vs_fp64(case):
    from rick_amd import cdc, dcl
    _, _, ra, rb, ref = _case(case)
    base = _xgram_err((ra @ rb.t(), torch.diagonal(ra @ ra.t()), torch.diagonal(rb @ rb.t())), ref)     # fp32 composition, CPU
    ad, bd = _to_dev(case)
    got = dcl.xgram(ad, bd)
    err = _xgram_err(got, ref)
    print(f'xgram {_ids(case)}: device {err:.3e}  fp32 composition {base:.3e}  bound {4 * base:.3e}')
    C, na, nb = got
    assert C.dtype == na.dtype == nb.dtype == torch.float64
    assert C.shape == (ra.shape[0], rb.shape[0]) and na.shape == (ra.shape[0],) and nb.shape == (rb.shape[0],)
    again = dcl.xgram(ad, bd)
    assert all(torch.equal(x, y) for x, y in zip(got, again))                    # run to run
    assert err <= 4 * base
    Ba, Bb = ra.shape[0], rb.shape[0]
    if Ba + Bb <= cdc.MAX_B:                                                     # the exactness oracle: rick_gram_f32 of the rows stacked
        cat = torch.cat([ad, bd])
        if ad.dim() == 4:
            cat = cat.contiguous(memory_format=torch.channels_last)
        G = cdc.gram(cat)
        assert torch.equal(C, G[:Ba, Ba:]) and torch.equal(na, torch.diagonal(G)[:Ba]) and torch.equal(nb, torch.diagonal(G)[Ba:])
    if case == 'mixed':                                                          # the scalar path: the same sums as the 16-byte path
        assert all(torch.equal(x, y) for x, y in zip(got, dcl.xgram(ad.clone(), bd)))
        assert all(torch.equal(x, y) for x, y in zip(dcl.xgram(bd, ad)[:1], (C.t(),)))      # b misaligned instead of a
    if case == 'halves':
        assert cdc._rows(bd).data_ptr() == bd.data_ptr() and cdc._sample_dense(ad) and dcl._same_layout(ad, bd)    # read in place


def test_xgram_entry_depends_on_its_two_rows_alone():
    from rick_amd import dcl
    ad, bd = _to_dev((8, 8, 8192))
    C, na, nb = dcl.xgram(ad, bd)
    for i in range(8):
        for j in range(8):
            c, p, q = dcl.xgram(ad[i:i + 1], bd[j:j + 1])
            assert torch.equal(c[0, 0], C[i, j]) and torch.equal(p[0], na[i]) and torch.equal(q[0], nb[j]), (i, j)
    c, p, q = dcl.xgram(ad[[5, 2, 7]], bd[[6, 0]])                               # other row counts, other addresses
    assert torch.equal(c, C[[5, 2, 7]][:, [6, 0]]) and torch.equal(p, na[[5, 2, 7]]) and torch.equal(q, nb[[6, 0]])


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_xrowmix_vs_fp64(case):
    from rick_amd import cdc, dcl
    _, _, ra, rb, _ = _case(case)
    Ba, Bb = ra.shape[0], rb.shape[0]
    ad, bd = _to_dev(case)
    rad, rbd = cdc._rows(ad), cdc._rows(bd)
    gen = torch.Generator().manual_seed(Ba * 8 + Bb)
    M, d = torch.randn(Ba, Bb, generator=gen), torch.randn(Ba, generator=gen)
    y = dcl.xrowmix(M.to(DEV), d.to(DEV), rad, rbd)                              # the kernel reads M and d from device memory
    ref = d.double()[:, None] * ra.double() + M.double() @ rb.double()
    scale = ref.abs().max()
    base = float(((d[:, None] * ra + M @ rb).double() - ref).abs().max() / scale)
    err = float((y.double().cpu() - ref).abs().max() / scale)
    print(f'xrowmix {_ids(case)}: device {err:.3e}  fp32 composition {base:.3e}  bound {4 * base:.3e}')
    assert err <= 4 * base
    # M = 0, d = 1: a bit for bit;  d = 0, M one-hot: that row of b bit for bit
    assert torch.equal(dcl.xrowmix(torch.zeros(Ba, Bb, device=DEV), torch.ones(Ba, device=DEV), rad, rbd), rad)
    pick = [(3 * k + 1) % Bb for k in range(Ba)]
    hot = torch.zeros(Ba, Bb, device=DEV)
    hot[torch.arange(Ba), pick] = 1.0
    assert torch.equal(dcl.xrowmix(hot, torch.zeros(Ba, device=DEV), rad, rbd), rbd[pick])


def test_xgram_backward_is_xrowmix_in_the_layout_of_each_operand():
    from rick_amd import dcl
    a, b, ra, rb, _ = _case('channels_last')
    ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    g = torch.Generator().manual_seed(0)
    w, u, v = (torch.randn(*s, dtype=torch.float64, generator=g) for s in ((3, 2), (3,), (2,)))
    C, na, nb = dcl.xgram(ad, bd)
    ga, gb = torch.autograd.grad((C * w.to(DEV)).sum() + (na * u.to(DEV)).sum() + (nb * v.to(DEV)).sum(), (ad, bd))
    assert ga.stride() == ad.stride() and ga.shape == ad.shape and gb.stride() == bd.stride() and gb.shape == bd.shape
    for got, rows, other, gc, gn in ((ga, ra, rb, w, u), (gb, rb, ra, w.t(), v)):
        shape = (rows.shape[0], 9, 7, 24)
        ref = (gc @ other.double() + 2 * gn[:, None] * rows.double()).view(shape).permute(0, 3, 1, 2)
        b32 = ((2 * gn).float()[:, None] * rows + gc.float() @ other).view(shape).permute(0, 3, 1, 2)
        base, err = float((b32.double() - ref).abs().max() / ref.abs().max()), float((got.double().cpu() - ref).abs().max() / ref.abs().max())
        print(f'xgram backward: device {err:.3e}  fp32 composition {base:.3e}')
        assert err <= 4 * base
    (only_a,) = torch.autograd.grad((dcl.xgram(ad, bd.detach())[0] * w.to(DEV)).sum(), ad)       # b needs no gradient: one launch
    assert only_a.stride() == ad.stride()
    with pytest.raises(RuntimeError, match='first order'):
        torch.autograd.grad(dcl.xgram(ad, bd)[0].sum(), ad, create_graph=True)


# ---- losses and gradients with respect to the features -------------------------------------------------------------------------
FEAT_SHAPES = [(8, 4, 4), (16, 8, 8), (5, 7, 9), (3, 33, 31)]
TAU = 0.07


def _cos32(A, X):
    """Cosines by matmul in the dtype of the operands: the base of the fourfold rule."""
    A, X = A.flatten(1), X.flatten(1)
    return (A @ X.t()) / ((A * A).sum(1).sqrt().clamp_min(1e-8)[:, None] * (X * X).sum(1).sqrt().clamp_min(1e-8)[None, :])


def cl1_composed(ft, fs, layers, dtype=torch.float32):
    terms = []
    for i, l in enumerate(layers):
        logp = torch.log_softmax(_cos32(ft[l].to(dtype), fs[l].detach().to(dtype)) / TAU, 1)
        terms.append(-logp[i, i])
    return torch.stack(terms).mean()


def cl2_composed(fa, fp, fx, layers, dtype=torch.float32):
    terms = []
    for i, l in enumerate(layers):
        a = fa[l].to(dtype)
        pos = torch.diagonal(_cos32(a, fp[l].detach().to(dtype)))
        logp = torch.log_softmax(torch.cat([pos[:, None], _cos32(a, fx[l].to(dtype))], 1) / TAU, 1)
        terms.append(-logp[i, 0])
    return torch.stack(terms).mean()


def _feats(seed):
    from tests.dcl_f64 import random_feats
    gen = torch.Generator().manual_seed(seed)
    pos = random_feats(FEAT_SHAPES, 4, seed)
    anc = [f + 0.3 * torch.randn(f.shape, generator=gen) for f in pos]
    neg = [torch.randn(4, *s, generator=gen) * 0.5 + f[:1] for f, s in zip(pos, FEAT_SHAPES)]
    for fl in (pos, anc, neg):
        fl[1] = fl[1].contiguous(memory_format=torch.channels_last)             # the networks' layout
    return anc, pos, neg


def _compare(name, layers, ref, gref, cpu, gcpu, loss, gdev, leaves):
    assert loss.dtype == torch.float32 and loss.dim() == 0
    err, base = abs(float(loss.detach()) - float(ref.detach())), abs(float(cpu.detach()) - float(ref.detach()))
    print(f'{name} {layers}: value {float(ref.detach()):.6e}  device err {err:.3e}  fp32 composition {base:.3e}')
    assert err <= 4 * base
    for k, (a, b, r, leaf) in enumerate(zip(gdev, gcpu, gref, leaves)):
        scale = r.abs().max()
        e, bs = float((a.double().cpu() - r).abs().max() / scale), float((b.double() - r).abs().max() / scale)
        print(f'  d {name} / d operand {k}: device {e:.3e}  fp32 composition {bs:.3e}  bound {4 * bs:.3e}')
        assert a.stride() == leaf.stride()
        assert e <= 4 * bs


@pytest.mark.parametrize('layers', [[0, 1, 2, 3], [2, 0, 2, 2]], ids=['distinct', 'repeated'])
def test_cl1_and_feature_gradients_vs_fp64(layers):
    from rick_amd import dcl
    from tests.dcl_f64 import cl1_f64
    tgt, src, _ = _feats(sum(layers))
    used = sorted(set(layers))
    t64 = [f.double().requires_grad_(True) for f in tgt]
    ref = cl1_f64(t64, src, layers, TAU)
    gref = torch.autograd.grad(ref, [t64[l] for l in used])
    t32 = [f.clone().requires_grad_(True) for f in tgt]
    cpu = cl1_composed(t32, src, layers)
    gcpu = torch.autograd.grad(cpu, [t32[l] for l in used])
    td = [f.to(DEV).requires_grad_(True) for f in tgt]
    loss = dcl.generator_contrastive_loss(td, [f.to(DEV) for f in src], layers, TAU)
    gdev = torch.autograd.grad(loss, [td[l] for l in used])
    _compare('CL1', layers, ref, gref, cpu, gcpu, loss, gdev, [td[l] for l in used])


@pytest.mark.parametrize('layers', [[0, 1, 2, 3], [3, 1, 3, 3]], ids=['distinct', 'repeated'])
def test_cl2_and_feature_gradients_vs_fp64(layers):
    from rick_amd import dcl
    from tests.dcl_f64 import cl2_f64
    anc, pos, neg = _feats(10 + sum(layers))
    used = sorted(set(layers))
    a64, n64 = [f.double().requires_grad_(True) for f in anc], [f.double().requires_grad_(True) for f in neg]
    ref = cl2_f64(a64, pos, n64, layers, TAU)
    gref = torch.autograd.grad(ref, [a64[l] for l in used] + [n64[l] for l in used])
    a32, n32 = [f.clone().requires_grad_(True) for f in anc], [f.clone().requires_grad_(True) for f in neg]
    cpu = cl2_composed(a32, pos, n32, layers)
    gcpu = torch.autograd.grad(cpu, [a32[l] for l in used] + [n32[l] for l in used])
    ad, nd = [f.to(DEV).requires_grad_(True) for f in anc], [f.to(DEV).requires_grad_(True) for f in neg]
    loss = dcl.discriminator_contrastive_loss(ad, [f.to(DEV) for f in pos], nd, layers, TAU)
    leaves = [ad[l] for l in used] + [nd[l] for l in used]                       # anchors, then the negatives
    gdev = torch.autograd.grad(loss, leaves)
    _compare('CL2', layers, ref, gref, cpu, gcpu, loss, gdev, leaves)


def test_cl1_of_one_sample_is_exactly_zero():
    from rick_amd import dcl
    tgt, src, _ = _feats(1)
    td = [f[:1].to(DEV).requires_grad_(True) for f in tgt]
    loss = dcl.generator_contrastive_loss(td, [f[:1].to(DEV) for f in src], [3], TAU)
    assert float(loss.detach()) == 0.0
    assert not torch.autograd.grad(loss, td[3])[0].any()
