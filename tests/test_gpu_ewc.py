"""rick_ewc_f32 / rick_ewc_finish_f64 (rick_amd/csrc/ewc.hip) and everything rick_amd/ewc.py builds on them against the NumPy fp64
restatement tests/ewc_f64.py; estimate_fisher against a loop of backward() calls; the trainer's G step with the term, eager,
captured, and behind a gradient exchange.

Bounds (tests/ewc_f64.py):
  gradient, per element: |g_dev - (g0 + 2 w F (theta - theta*))| <= 3 * 2^-24 (|g0| + |2 w F (theta - theta*)|): the kernel's three
      fp32 roundings (difference, product, FMA) against exact fp64 operands.
  value: |v_dev - v| <= n * 2^-52 * v: n non-negative fp64 products, each rounded once; a term passes through at most
      16 + 3 + 6 + 3 additions inside its block and ceil(blocks / 256) + 9 in the finishing launch, far fewer than the n - 1 of the
      bound for every n > 2; at n <= 2 the lanes add zeros, which is exact, and the restatement's fsum adds one rounding.
The figures each test prints (run with -s) are the measured errors as fractions of these bounds."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch

from tests import ewc_f64

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# one element; fewer than a float4; a partial block; one short of a block, a block, one more; three blocks and a tail; 256 blocks
SIZES = [1, 3, 255, 4095, 4096, 4097, 3 * 4096 + 5, 1 << 20]
WEIGHTS = [1.0, 5e8 * 1e-8]
_cache = {}


def _case(n, off=0, seed=None):
    """theta, theta*, F, g0 (NumPy fp32, n elements) and the fp64 value — computed once per (n, off) and shared.  F is drawn from
    {0} and log-uniformly from [1e-8, 1e-2]; theta - theta* is of order 1e-2; g0 ~ N(0, 1)."""
    key = (n, off, seed)
    if key not in _cache:
        rng = np.random.RandomState(n % 100003 + 7 * off if seed is None else seed)
        anchor = rng.standard_normal(n).astype(np.float32)
        theta = (anchor + 1e-2 * rng.standard_normal(n)).astype(np.float32)
        fisher = np.where(rng.rand(n) < 0.1, 0.0, 10.0 ** rng.uniform(-8, -2, n)).astype(np.float32)
        if n > 2:
            fisher[[0, n - 1]] = 1e-2, 1e-8                    # the ends of the range are present, the first and last element count
        g0 = rng.standard_normal(n).astype(np.float32)
        _cache[key] = dict(theta=theta, anchor=anchor, fisher=fisher, g0=g0, value=ewc_f64.value(theta, anchor, fisher))
    return _cache[key]


def _dev(x, off, pad=5):
    """x on the device at `off` elements past a 16-byte boundary, with guard elements on both sides; returns (view, whole)."""
    whole = torch.full((off + x.size + pad + 4,), 7.0 if x.dtype != np.uint8 else 9, dtype=torch.from_numpy(x[:0]).dtype, device=DEV)
    assert whole.data_ptr() % 16 == 0
    view = whole[4 + off:4 + off + x.size]
    view.copy_(torch.from_numpy(x))
    return view, whole


def _guards_intact(view_whole, off, n, fill):
    _, whole = view_whole
    return bool((whole[:4 + off] == fill).all()) and bool((whole[4 + off + n:] == fill).all())


def _run(c, off, weight, mask=None, offs=None):
    from rick_amd.ewc import accumulate_
    offs = offs or {}
    t = {k: _dev(c[k], offs.get(k, off)) for k in ('theta', 'anchor', 'fisher', 'g0')}
    m = _dev(mask, offs.get('mask', off)) if mask is not None else None
    v = accumulate_(t['theta'][0], t['anchor'][0], t['fisher'][0], t['g0'][0], weight, mask=None if m is None else m[0])
    torch.cuda.synchronize()
    n = c['theta'].size
    assert all(_guards_intact(t[k], offs.get(k, off), n, 7.0) for k in t)          # nothing written outside [0, n)
    assert torch.equal(t['theta'][0].cpu(), torch.from_numpy(c['theta'])) and torch.equal(t['fisher'][0].cpu(), torch.from_numpy(c['fisher']))
    return v, t['g0'][0]


def _check(c, v, g, weight, mask=None, what=''):
    n = c['theta'].size
    term = ewc_f64.grad_term(c['theta'], c['anchor'], c['fisher'], weight, mask)
    vref = c['value'] if mask is None else ewc_f64.value(c['theta'], c['anchor'], c['fisher'], mask)
    gerr = np.abs(g.cpu().numpy().astype(np.float64) - (c['g0'].astype(np.float64) + term))
    gb = ewc_f64.grad_bound(c['g0'], term)
    verr, vb = abs(float(v) - vref), ewc_f64.value_bound(n, vref)
    print(f'ewc {what} n={n} w={weight:g}: gradient error / bound {float((gerr / gb).max()):.3f}, value {vref:.6e} error {verr:.3e} '
          f'bound {vb:.3e}')
    assert v.dtype == torch.float64 and v.dim() == 0
    assert (gerr <= gb).all()
    assert verr <= vb


@pytest.mark.parametrize('off', [0, 1, 2, 3])
@pytest.mark.parametrize('n', SIZES)
def test_kernel_vs_fp64(n, off):
    c = _case(n, off)
    for w in WEIGHTS:
        v, g = _run(c, off, w)
        _check(c, v, g, w, what=f'off={off}')


@pytest.mark.parametrize('n', [255, 4097, 3 * 4096 + 5])
def test_kernel_streams_at_different_phases(n):
    """The four streams (and the mask) each at another offset from a 16-byte boundary: the element-by-element form."""
    c = _case(n)
    offs = dict(theta=1, anchor=0, fisher=3, g0=2, mask=1)
    mask = np.random.RandomState(n).randint(0, 4, n).astype(np.uint8)
    v, g = _run(c, 0, 1.0, offs=offs)
    _check(c, v, g, 1.0, what='mixed phases')
    v, g = _run(c, 0, 1.0, mask=mask, offs=offs)
    _check(c, v, g, 1.0, mask=mask, what='mixed phases, mask')


@pytest.mark.parametrize('n,off', [(3 * 4096 + 5, 0), (3 * 4096 + 5, 3), (1 << 20, 0)])
def test_two_runs_are_identical(n, off):
    c = _case(n, off)
    v1, g1 = _run(c, off, 5.0)
    v2, g2 = _run(c, off, 5.0)
    assert torch.equal(v1, v2) and torch.equal(g1, g2)


@pytest.mark.parametrize('n,off', [(4097, 0), (4097, 1), (3 * 4096 + 5, 2)])
def test_zero_fisher_zero_difference_zero_weight(n, off):
    c = _case(n, off)
    g0 = torch.from_numpy(c['g0'])
    v, g = _run(dict(c, fisher=np.zeros_like(c['fisher'])), off, 5.0)
    assert float(v) == 0.0 and torch.equal(g.cpu(), g0)
    v, g = _run(dict(c, anchor=c['theta']), off, 5.0)
    assert float(v) == 0.0 and torch.equal(g.cpu(), g0)
    v, g = _run(c, off, 0.0)
    assert torch.equal(g.cpu(), g0)
    assert abs(float(v) - c['value']) <= ewc_f64.value_bound(n, c['value']) and c['value'] > 0
    assert torch.equal(v, _run(c, off, 1.0)[0])                # the value does not depend on the weight


@pytest.mark.parametrize('n,off', [(3, 0), (4097, 0), (3 * 4096 + 5, 1), (3 * 4096 + 5, 3)])
def test_masked_elements_neither_pull_nor_count(n, off):
    c = _case(n, off)
    mask = np.random.RandomState(n + off).randint(0, 4, n).astype(np.uint8)
    mask[:2] = 1, 0
    v, g = _run(c, off, 5.0, mask=mask)
    _check(c, v, g, 5.0, mask=mask, what=f'mask off={off}')
    keep = ewc_f64.kept(mask, n)
    bits, bits0 = g.cpu().numpy().view(np.int32), c['g0'].view(np.int32)
    assert np.array_equal(bits[~keep], bits0[~keep])           # bit patterns kept
    moved = keep & (c['fisher'] > 1e-4) & (c['theta'] != c['anchor'])      # a term of order 1e-5 or more against g0 ~ N(0, 1)
    assert n < 100 or (moved.any() and (bits[moved] != bits0[moved]).mean() > 0.5)
    # all masked: nothing counts, nothing moves
    v, g = _run(c, off, 5.0, mask=np.full(n, 2, dtype=np.uint8))
    assert float(v) == 0.0 and np.array_equal(g.cpu().numpy().view(np.int32), bits0)
    # bits other than freeze (1) and prune (2) do not mask
    v4, g4 = _run(c, off, 5.0, mask=np.full(n, 4, dtype=np.uint8))
    v0, g0 = _run(c, off, 5.0)
    assert torch.equal(v4, v0) and torch.equal(g4, g0)


def test_n_zero_writes_zero():
    from rick_amd._lib import check, lib, ptr, stream_ptr
    from rick_amd.ewc import accumulate_
    x = torch.full((8,), 3.0, device=DEV)
    partials = torch.full((4,), float('nan'), device=DEV, dtype=torch.float64)
    out = torch.full((), float('nan'), device=DEV, dtype=torch.float64)
    assert lib.rick_ewc_blocks(0) == 0
    check(lib.rick_ewc_f32(ptr(x), ptr(x), ptr(x), ptr(x), None, 0, 1.0, ptr(partials), stream_ptr()), 'rick_ewc_f32')
    check(lib.rick_ewc_finish_f64(ptr(partials), 0, ptr(out), stream_ptr()), 'rick_ewc_finish_f64')
    assert float(out) == 0.0 and bool((x == 3.0).all()) and bool(torch.isnan(partials).all())
    e = x[:0]
    assert float(accumulate_(e, e, e, e.clone(), 1.0)) == 0.0


def test_blocks_matches_the_partials_the_pass_writes():
    from rick_amd._lib import lib
    from rick_amd.ewc import accumulate_
    ns = [1, 4095, 4096, 4097, 3 * 4096 + 5]
    counts = [lib.rick_ewc_blocks(n) for n in range(0, 4 * 4096 + 2)]
    assert counts == sorted(counts) and counts[0] == 0 and counts[1] == 1 and counts[-1] == 5
    for n in ns:
        c = _case(n)
        blocks = lib.rick_ewc_blocks(n)
        partials = torch.full((blocks + 8,), float('nan'), device=DEV, dtype=torch.float64)
        t = [torch.from_numpy(c[k]).to(DEV) for k in ('theta', 'anchor', 'fisher', 'g0')]
        v = accumulate_(*t, 1.0, partials=partials)
        assert bool(torch.isfinite(partials[:blocks]).all()) and bool(torch.isnan(partials[blocks:]).all())
        assert torch.isfinite(v) and abs(float(v) - c['value']) <= ewc_f64.value_bound(n, c['value'])
        assert bool((partials[:blocks] >= 0).all()) and (n < 4096 or bool((partials[:blocks] > 0).all()))


# ---- networks ------------------------------------------------------------------------------------------------------------------
def _build(size=32):
    from rick_amd.models import Discriminator, Generator
    torch.manual_seed(11)
    g0, d0 = Generator(size, 512, 2), Discriminator(size)

    def make(perturb=0.0):
        g, d = Generator(size, 512, 2), Discriminator(size)
        g.load_state_dict(g0.state_dict())
        d.load_state_dict(d0.state_dict())
        if perturb:
            gen = torch.Generator().manual_seed(1)
            with torch.no_grad():
                for n, p in g.named_parameters():
                    if n.startswith('convs.'):
                        p.add_(perturb * p.abs().mean() * torch.randn(p.shape, generator=gen))
        return g.to(DEV), d.to(DEV)
    return make, {k: v.detach().clone().to(DEV) for k, v in g0.state_dict().items()}


def _noise_maps(g):
    gen = torch.Generator(DEV).manual_seed(2)
    return [torch.randn(n.shape, device=DEV, generator=gen) for n in g.make_noise()]


def test_estimate_fisher_vs_backward_loop():
    """32 px, 3 latents, the generator's stored noise maps: the mean of grad^2 of the non-saturating loss at batch 1.  Per element
    samples + 1 fp32 roundings of non-negative terms (one FMA per sample, one division), against the fp64 mean of the same
    gradients taken by backward()."""
    from rick_amd.ewc import estimate_fisher
    from rick_amd.train import g_nonsaturating_loss, g_optim_filter
    make, _ = _build()
    g, d = make(perturb=0.3)
    flags = {id(p): p.requires_grad for net in (g, d) for p in net.parameters()}
    zs = [torch.randn(512, device=DEV, generator=torch.Generator(DEV).manual_seed(20 + k)) for k in range(3)]
    fisher = estimate_fisher(g, d, zs, fixed_noise=True)
    opt = [(n, p) for n, p in g.named_parameters() if g_optim_filter(n)]
    assert list(fisher) == [n for n, _ in opt]
    assert all(p.requires_grad == flags[id(p)] for net in (g, d) for p in net.parameters())
    assert all(p.grad is None for p in g.parameters())
    # the loop: the discriminator's weights need no gradients here either (its data gradients are the same kernels)
    for p in d.parameters():
        p.requires_grad = False
    ref = {n: torch.zeros(p.shape, device=DEV, dtype=torch.float64) for n, p in opt}
    for z in zs:
        for p in g.parameters():
            p.grad = None
        fake, _ = g([z.view(1, -1)], randomize_noise=False)
        pred, _ = d(fake)
        g_nonsaturating_loss(pred).backward()
        for n, p in opt:
            if p.grad is not None:
                ref[n] += p.grad.double() ** 2
    worst, live = 0.0, 0
    for n, _ in opt:
        r = ref[n] / len(zs)
        assert fisher[n].shape == r.shape and fisher[n].dtype == torch.float32 and bool((fisher[n] >= 0).all())
        err = (fisher[n].double() - r).abs()
        assert bool((err <= (len(zs) + 1) * ewc_f64.U32 * r).all()), n
        if bool(r.any()):
            live += 1
            worst = max(worst, float((err / r.clamp_min(1e-300)).max()) / ((len(zs) + 1) * ewc_f64.U32))
    print(f'estimate_fisher: {live} of {len(opt)} tensors with a gradient, worst relative error / bound {worst:.3f}')
    assert live >= 8


def _trainer(make, state, weight, dp=None, seed=4):
    """32 px, batch 2; the generator has moved away (0.3 mean |w| per weight) from the source state the anchor holds; F uniform in
    [0, 1e-2)."""
    from rick_amd.train import RickTrainer, TrainConfig
    g, d = make(perturb=0.3)
    g_ema, d_ema = make()
    gen = torch.Generator(DEV).manual_seed(seed)
    fis = {n: 1e-2 * torch.rand(p.shape, device=DEV, generator=gen) for n, p in g.named_parameters()}
    cfg = TrainConfig(size=32, batch=2, n_mlp=2, warmup_iter=0, ewc_weight=weight)
    return RickTrainer(cfg, g, d, g_ema, d_ema, dp=dp, ewc=(state, fis) if weight > 0 else None)


def _fixed(g):
    gen = torch.Generator(DEV).manual_seed(7)
    return dict(noise=[torch.randn(2, 512, device=DEV, generator=gen)], g_noise=_noise_maps(g),
                plr_noise=[torch.randn(1, 512, device=DEV, generator=gen)], pl_noise=torch.randn(1, 3, 32, 32, device=DEV, generator=gen))


def _np(t):
    return t.detach().cpu().numpy()


def test_g_step_eager_adds_the_term_and_plr_step_does_not():
    make, state = _build()
    w = 50.0
    a, b = _trainer(make, state, 0.0), _trainer(make, state, w)
    fx = _fixed(a.g)
    lo, hi = b.ewc.lo, b.ewc.hi
    assert torch.equal(a.g_flat.flat, b.g_flat.flat)
    # the path-length step first, from the common state: no term, the same gradient bit for bit
    for tr in (a, b):
        tr.plr_step(fx['plr_noise'], pl_noise=fx['pl_noise'], g_noise=fx['g_noise'])
    assert 'ewc' not in b.losses
    assert bool(a.g_flat.grad[lo:hi].any()) and torch.equal(a.g_flat.grad, b.g_flat.grad) and torch.equal(a.g_flat.flat, b.g_flat.flat)
    # the G step
    theta = _np(b.g_flat.flat[lo:hi]).copy()
    for tr in (a, b):
        tr.g_step(fx['noise'], fx['g_noise'])
    assert 'ewc' not in a.losses and torch.equal(a.losses['g'], b.losses['g'])
    ga, gb = _np(a.g_flat.grad[lo:hi]), _np(b.g_flat.grad[lo:hi])
    term = ewc_f64.grad_term(theta, _np(b.ewc.anchor), _np(b.ewc.fisher), w)
    err, bound = np.abs(gb.astype(np.float64) - (ga.astype(np.float64) + term)), ewc_f64.grad_bound(ga, term)
    vref = ewc_f64.value(theta, _np(b.ewc.anchor), _np(b.ewc.fisher))
    verr, vb = abs(float(b.losses['ewc']) - vref), ewc_f64.value_bound(hi - lo, vref)
    print(f'g_step: gradient error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}; term / gradient (max) '
          f'{np.abs(term).max() / np.abs(ga).max():.3f}; value {vref:.6e} error {verr:.3e} bound {vb:.3e}')
    assert (err <= bound).all()
    assert np.abs(term).max() > 1e-2 * np.abs(ga).max()        # the term is a visible part of the gradient it is checked in
    assert b.losses['ewc'].dtype == torch.float64 and vref > 0 and verr <= vb
    assert torch.equal(a.g_flat.grad[:lo], b.g_flat.grad[:lo]) and torch.equal(a.g_flat.grad[hi:], b.g_flat.grad[hi:])
    assert not torch.equal(a.g_flat.flat, b.g_flat.flat)       # ... and of the update
    assert b.g_optim.before_step is None
    # a later path-length step leaves the value alone
    held, before = b.losses['ewc'], b.losses['ewc'].clone()
    b.plr_step(fx['plr_noise'], pl_noise=fx['pl_noise'], g_noise=fx['g_noise'])
    assert b.losses['ewc'] is held and torch.equal(held, before)


def test_g_step_graph_reads_live_buffers_and_refreshes_the_value():
    make, state = _build()
    tr = _trainer(make, state, 50.0)
    tr.enable_graphs(True)
    a = tr.ewc
    anchor, fisher = _np(a.anchor), _np(a.fisher)
    values = []
    for k in range(5):                                         # two eager warm-up steps, the capture, two replays
        theta = _np(tr.g_flat.flat[a.lo:a.hi]).copy()
        tr.g_step(None, graph=True)
        vref = ewc_f64.value(theta, anchor, fisher)
        verr, vb = abs(float(tr.losses['ewc']) - vref), ewc_f64.value_bound(a.n, vref)
        print(f'graph step {k}: value {vref:.6e} error {verr:.3e} bound {vb:.3e}')
        assert verr <= vb
        values.append(vref)
    assert len(set(values)) == 5                               # the parameters moved every step, and the value with them
    graphs = tr._gs['g']['graphs']
    assert graphs[1] is not None and 'ewc' in tr._gs['g']['losses']
    # another Fisher, loaded in place: the next replay follows it without a new capture
    sd = a.state_dict()
    for k in sd:
        if k.startswith('fisher.'):
            sd[k] = sd[k] * 3 + 1e-3
    ptrs = (a.anchor.data_ptr(), a.fisher.data_ptr())
    a.load_state_dict(sd)
    assert ptrs == (a.anchor.data_ptr(), a.fisher.data_ptr())
    theta = _np(tr.g_flat.flat[a.lo:a.hi]).copy()
    tr.g_step(None, graph=True)
    assert tr._gs['g']['graphs'] is graphs
    vref = ewc_f64.value(theta, anchor, _np(a.fisher))
    assert vref > 2 * values[-1] and abs(float(tr.losses['ewc']) - vref) <= ewc_f64.value_bound(a.n, vref)


def _dp_worker(q, port):
    """One rank on the 'nccl' backend with forced collectives, eager (gradient hooks launch the bucket all-reduces while backward
    runs): one G step with the term, next to the plain trainer from the same state and inputs.  Then four G steps with step
    graphs, where the optimiser part of the split capture is deferred behind the exchange."""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0',
                      HSA_ENABLE_IPC_MODE_LEGACY='0')
    import random

    import torch.distributed as dist
    from rick_amd.dist import DataParallelGrads
    torch.cuda.set_device(0)
    dist.init_process_group('nccl', rank=0, world_size=1)
    make, state = _build()
    out = {}
    for mode in ('plain', 'dp', 'off'):
        dp = DataParallelGrads(bucket_bytes=256 * 1024, force=True) if mode == 'dp' else None
        tr = _trainer(make, state, 0.0 if mode == 'off' else 50.0, dp=dp)
        if dp is not None:
            assert dp.active and dp.hooks_enabled and len(dp._state[id(tr.g_flat)]['buckets']) >= 3
        fx = _fixed(tr.g)
        tr.g_step(fx['noise'], fx['g_noise'])
        torch.cuda.synchronize()
        out[mode] = (tr.g_flat.flat.detach().clone(), float(tr.losses['ewc']) if mode != 'off' else None)
    res = {'equal': bool(torch.equal(out['plain'][0], out['dp'][0])), 'value': (out['plain'][1], out['dp'][1]),
           'term_moves': not bool(torch.equal(out['plain'][0], out['off'][0])), 'finite': bool(torch.isfinite(out['dp'][0]).all())}
    # the same pair with step graphs: under data parallelism the capture is split (head | forward/backward | optimiser) and the
    # term's launches belong to the third graph, replayed once the exchange has completed
    for mode in ('plain', 'dp'):
        random.seed(3)
        torch.manual_seed(3)
        dp = DataParallelGrads(bucket_bytes=256 * 1024, force=True) if mode == 'dp' else None
        tr = _trainer(make, state, 50.0, dp=dp)
        tr.enable_graphs(True)
        values = []
        for _ in range(4):                                     # two eager warm-up steps, the capture, one replay
            tr.g_step(None, graph=True)
            tr.ema_step()                                      # completes the deferred optimiser graph
            values.append(float(tr.losses['ewc']))
        if dp is not None:
            res['split'] = all(g is not None for g in tr._gs['g']['graphs'])
        torch.cuda.synchronize()
        out[mode] = (tr.g_flat.flat.detach().clone(), values)
    res['graph_equal'] = bool(torch.equal(out['plain'][0], out['dp'][0]))
    res['graph_values'] = (out['plain'][1], out['dp'][1])
    dist.destroy_process_group()
    q.put(res)


def test_single_rank_data_parallel_steps_equal_the_plain_ones():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    p = ctx.Process(target=_dp_worker, args=(q, port))
    p.start()
    try:
        out = q.get(timeout=300)
    finally:
        p.join(60)
        if p.is_alive():
            p.kill()
    assert p.exitcode == 0
    assert out['equal'] and out['finite'] and out['term_moves'], out
    assert out['value'][0] == out['value'][1] and out['value'][0] > 0
    assert out['split'] and out['graph_equal'], out
    assert out['graph_values'][0] == out['graph_values'][1] and len(set(out['graph_values'][0])) == 4
