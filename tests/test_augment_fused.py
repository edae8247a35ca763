"""Adaptive discriminator augmentation on the fused HIP kernels (rick_amd/csrc/augment.hip): the host side (retry loop, pads,
parameter block), the ADA controller of the trainer and its config (CPU); forward parity with the reference fixtures and the
composed path, the adjoint, determinism (GPU)."""
import math

import numpy as np
import pytest
import torch


# ----------------------------------------------------------------------------------------------------------------- CPU
def test_train_config_has_the_reference_augment_flags():
    from rick_amd.train import TrainConfig
    cfg = TrainConfig()
    assert (cfg.augment, cfg.augment_p, cfg.ada_target, cfg.ada_length) == (False, 0.0, 0.6, 500_000)


def _reference_ada(signs_and_sizes, target, length, p0=0.0):
    """Direct transcription of train_dynamic_update_prune.py:440-459 (one entry per D step: (sum of signs, batch))."""
    ada_aug_p, ada_aug_step, acc = p0, target / length, [0.0, 0]
    out = []
    for s, n in signs_and_sizes:
        acc = [acc[0] + s, acc[1] + n]
        if acc[1] > 255:
            pred_signs, n_pred = acc
            sign = 1 if pred_signs / n_pred > target else -1
            ada_aug_p += sign * ada_aug_step * n_pred
            ada_aug_p = min(1, max(0, ada_aug_p))
            acc = [0.0, 0]
        out.append(ada_aug_p)
    return out


@pytest.mark.parametrize('length', [500_000, 500])
def test_ada_controller_follows_the_reference_trajectory(length):
    from rick_amd.train import AdaController, TrainConfig
    rng = np.random.default_rng(5)
    seq = []
    for k in range(1200):       # long runs of positive, then negative logits: p climbs to the 1 clamp and falls to the 0 clamp
        n = int(rng.choice([4, 8, 16]))
        frac = 0.95 if (k // 300) % 2 == 0 else 0.1
        seq.append((float(sum(1 if rng.random() < frac else -1 for _ in range(n))), n))
    want = _reference_ada(seq, 0.6, length)
    ctl = AdaController(TrainConfig(augment=True, ada_length=length))
    got = []
    for s, n in seq:
        acc = getattr(ctl, '_test_acc', 0.0) + s
        ctl._test_acc = acc
        if ctl.due(n):
            ctl.update(acc)
            ctl._test_acc = 0.0
        got.append(ctl.p)
    assert np.allclose(got, want, rtol=0, atol=1e-12)
    if length == 500:
        assert max(want) == 1 and min(want[300:]) == 0        # both clamps were exercised


def test_ada_controller_fixed_p_never_moves():
    from rick_amd.train import AdaController, TrainConfig
    ctl = AdaController(TrainConfig(augment=True, augment_p=0.3))
    assert not any(ctl.due(64) for _ in range(100)) and ctl.p == 0.3


def test_retry_loop_draws_the_composed_paths_G_sequence():
    """A 16 px image at p = 1: many draws need a reflect pad the image cannot give and are redrawn.  The fused path's explicit
    check must accept and reject exactly the draws F.pad(mode='reflect') accepts and rejects."""
    import rick_amd.augment as A
    img = torch.rand(4, 3, 16, 16)
    calls = []
    sample = A.sample_affine

    def counted(*a, **k):
        calls.append(1)
        return sample(*a, **k)
    A.sample_affine = counted
    try:
        retried = 0
        for seed in range(6):
            torch.manual_seed(seed)
            calls.clear()
            _, Gc = A.random_apply_affine(img, 1.0)
            n_composed = len(calls)
            after_composed = torch.rand(1)
            torch.manual_seed(seed)
            calls.clear()
            Gf, pads = A.draw_affine(1.0, 4, 16, 16)
            assert len(calls) == n_composed and A.pads_ok(pads, 16, 16)
            assert torch.equal(Gc, Gf) and torch.equal(torch.rand(1), after_composed)
            retried += n_composed > 1
    finally:
        A.sample_affine = sample
    assert retried >= 3, retried          # the explicit check did reject draws (for most seeds)


def _grid_ix(G, h, w, pads, X, Y):
    """The composed path's sampling position (random_apply_affine's grid, grid_sample's align_corners=False unnormalisation)
    of warped-canvas pixel (X, Y), in float64."""
    px1, px2, py1, py2 = pads
    Wp, Hp = w + px1 + px2 + 12, h + py1 + py2 + 12
    wp, hp, W2, H2 = Wp - 11, Hp - 11, 2 * Wp - 11, 2 * Hp - 11
    xs = -2 * px1 / w - 1 + X * (2 * (wp - px1) / w - 1 - (-2 * px1 / w - 1)) / (W2 - 1)
    ys = -2 * py1 / h - 1 + Y * (2 * (hp - py1) / h - 1 - (-2 * py1 / h - 1)) / (H2 - 1)
    m = torch.inverse(G.float()).double()[:2]
    gx = (m[0, 0] * xs + m[0, 1] * ys + m[0, 2]) * (w / wp) + (w + 2 * px1) / wp - 1
    gy = (m[1, 0] * xs + m[1, 1] * ys + m[1, 2]) * (h / hp) + (h + 2 * py1) / hp - 1
    return float(((gx + 1) * W2 - 1) / 2), float(((gy + 1) * H2 - 1) / 2)


@pytest.mark.parametrize('angle', [0.0, 0.7])
def test_parameter_block_for_identity_and_rotated_G(angle):
    from rick_amd.augment import PARAM_DTYPE, _padding, aug_params
    h, w = 24, 40
    c, s = math.cos(angle), math.sin(angle)
    G = torch.tensor([[[c, -s, 0.1], [s, c, -0.05], [0, 0, 1.0]]]) if angle else torch.eye(3).unsqueeze(0)
    C = torch.arange(16, dtype=torch.float32).view(1, 4, 4)
    pads = _padding(torch.inverse(G), h, w)
    if not angle:
        assert pads == (0, 0, 0, 0)
    else:
        assert min(pads) > 0
    blk = aug_params(G, C, h, w, pads)
    assert blk.dtype == PARAM_DTYPE and blk.shape == (1,) and blk.nbytes == 144
    px1, px2, py1, py2 = pads
    assert (blk['px1'][0], blk['py1'][0], blk['wp'][0], blk['hp'][0]) == (px1, py1, w + px1 + px2 + 12, h + py1 + py2 + 12)
    assert np.array_equal(blk['col'][0], C[0, :3].reshape(-1).numpy())
    a = blk['a'][0]
    for r, cc in ((0, 0), (5, 17), (2 * h + 9, 2 * w + 9)):
        ix, iy = _grid_ix(G[0], h, w, pads, 2 * px1 + cc, 2 * py1 + r)
        assert abs(a[0] * cc + a[1] * r + a[2] - ix) < 1e-9 and abs(a[3] * cc + a[4] * r + a[5] - iy) < 1e-9
    inv = blk['ainv'][0].reshape(2, 2) @ np.array([[a[0], a[1]], [a[3], a[4]]])
    assert np.allclose(inv, np.eye(2), atol=1e-12)


def test_augment_symbols_are_exported():
    from rick_amd._lib import lib
    for name in ('rick_augment_workspace_floats', 'rick_augment_fwd_f32', 'rick_augment_adj_f32'):
        assert hasattr(lib, name), name
    assert lib.rick_augment_workspace_floats(2, 32, 24) == 2 * 3 * 74 * 58


# ----------------------------------------------------------------------------------------------------------------- GPU
def _random_case(n, h, w, seed, calls=1, G=None):
    from rick_amd.augment import aug_params, draw_affine, sample_color
    torch.manual_seed(seed)
    x = torch.rand(n * calls, 3, h, w, dtype=torch.float64) * 2 - 1
    Gs, Cs, pads, blocks = [], [], [], []
    for _ in range(calls):
        g, pd = draw_affine(1.0, n, h, w, G)
        c = torch.randn(n, 4, 4) * 0.5 + torch.eye(4)
        Gs.append(g), Cs.append(c), pads.append(pd), blocks.append(aug_params(g, c, h, w, pd))
    return x, Gs, Cs, pads, np.concatenate(blocks)


def _composed(x, G, C):
    from rick_amd.augment import apply_color, random_apply_affine
    return apply_color(random_apply_affine(x, 1.0, G)[0], C)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['a', 'b', 'c'])
def test_fused_matches_reference_fixtures(golden, tag):
    from rick_amd.augment import _padding, aug_params, augment_fused, upload_params
    g = golden('ada')
    img = torch.from_numpy(g[f'aug{tag}/img']).cuda()
    G, C = torch.from_numpy(g[f'aug{tag}/G']), torch.from_numpy(g[f'aug{tag}/C'])
    h, w = img.shape[2:]
    prm = upload_params(aug_params(G, C, h, w, _padding(torch.inverse(G.float()), h, w)), img.device)
    out = augment_fused(img, prm).cpu().numpy()
    ref = g[f'aug{tag}/out']
    assert np.abs(out - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize('size,n,calls', [(32, 3, 1), (64, 2, 2), (256, 2, 1)])
def test_fused_matches_composed_fp64(size, n, calls):
    """Random G / C at p = 1; calls = 2: one launch over two reference calls with different batch-maximum pads."""
    from rick_amd.augment import augment_fused, upload_params
    x, Gs, Cs, pads, blk = _random_case(n, size, size, 40 + size, calls)
    if calls == 2:
        assert pads[0] != pads[1]
    ref = torch.cat([_composed(x[k * n:(k + 1) * n], Gs[k], Cs[k]) for k in range(calls)])
    out = augment_fused(x.float().cuda(), upload_params(blk, 'cuda')).double().cpu()
    # the composed path builds its grid from fp32 linspace (canvas coordinates up to ~6 * size): a few 1e-6 of a pixel per 32 px
    tol = 2e-5 * (size / 32) * max(1.0, float(ref.abs().max()))
    assert float((out - ref).abs().max()) < tol


@pytest.mark.gpu
def test_fused_matches_composed_where_the_footprint_reaches_the_canvas_edge():
    """A zoom with a shift whose pads stay small: bilinear corners of the warped region fall outside the up-sampled canvas
    (grid_sample's zero padding), checked on the host from the parameter block before the comparison."""
    from rick_amd.augment import augment_fused, upload_params
    G = torch.tensor([[[1.1, 0, 0.2], [0, 1.1, 0.1], [0, 0, 1.0]]]).repeat(2, 1, 1)
    x, Gs, Cs, pads, blk = _random_case(2, 48, 48, 7, 1, G=G)
    a, H2, W2 = blk['a'][0], 2 * blk['hp'][0] - 11, 2 * blk['wp'][0] - 11
    r, cc = np.meshgrid(np.arange(2 * 48 + 10), np.arange(2 * 48 + 10), indexing='ij')
    ix, iy = a[0] * cc + a[1] * r + a[2], a[3] * cc + a[4] * r + a[5]
    assert ((ix < 0) | (ix >= W2 - 1) | (iy < 0) | (iy >= H2 - 1)).any()
    ref = _composed(x, Gs[0], Cs[0])
    out = augment_fused(x.float().cuda(), upload_params(blk, 'cuda')).double().cpu()
    assert float((out - ref).abs().max()) < 4e-5 * max(1.0, float(ref.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize('size,calls', [(32, 2), (40, 1)])
def test_adjoint_identity_and_gradient_against_composed_autograd(size, calls):
    from rick_amd.augment import AugmentAdjFn, AugmentFn, upload_params
    x, Gs, Cs, pads, blk = _random_case(2, size, size, 90 + size, calls)
    prm = upload_params(blk, 'cuda')
    y = torch.randn_like(x)
    ax = AugmentFn.apply(x.float().cuda(), prm, False).double()
    aty = AugmentAdjFn.apply(y.float().cuda(), prm).double()
    lhs, rhs = float((ax.cpu() * y).sum()), float((x * aty.cpu()).sum())
    assert abs(lhs - rhs) < 1e-5 * (float((ax.cpu().abs() * y.abs()).sum()) + 1)
    # gradient of the fused op vs torch autograd of the composed path in fp64
    xr = x.clone().requires_grad_(True)
    ref = torch.cat([_composed(xr[k * 2:(k + 1) * 2], Gs[k], Cs[k]) for k in range(calls)])
    (gref,) = torch.autograd.grad((ref * y).sum(), xr)
    xf = x.float().cuda().requires_grad_(True)
    (gf,) = torch.autograd.grad((AugmentFn.apply(xf, prm, True) * y.float().cuda()).sum(), xf)
    assert float((gf.double().cpu() - gref).abs().max()) < 1e-4 * max(1.0, float(gref.abs().max()))
    # closed under differentiation: the gradient of the adjoint is the forward map without the colour offset
    v = torch.randn(x.shape, device='cuda')
    yr = y.float().cuda().requires_grad_(True)
    (gy,) = torch.autograd.grad((AugmentAdjFn.apply(yr, prm) * v).sum(), yr)
    assert torch.equal(gy, AugmentFn.apply(v, prm, False))


@pytest.mark.gpu
def test_fused_forward_and_adjoint_are_bitwise_reproducible_next_to_a_busy_neighbour():
    import os
    import subprocess
    import sys
    from rick_amd.augment import AugmentAdjFn, AugmentFn, upload_params
    x, _, _, _, blk = _random_case(4, 64, 64, 3, 2)
    prm = upload_params(blk, 'cuda')
    xf, yf = x.float().cuda(), torch.randn(8, 3, 64, 64, device='cuda')
    f0, a0 = AugmentFn.apply(xf, prm, True), AugmentAdjFn.apply(yf, prm)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    agg = subprocess.Popen([sys.executable, os.path.join(root, 'tools', 'stress_ops.py'), '--role', 'aggressor', '--seconds', '120'],
                           stdout=subprocess.PIPE, text=True)
    differing = 0
    try:
        for line in agg.stdout:
            if 'ready' in line:
                break
        assert agg.poll() is None, 'the neighbour process died before it started'
        for _ in range(200):
            f1, a1 = AugmentFn.apply(xf, prm, True), AugmentAdjFn.apply(yf, prm)
            differing += int(not torch.equal(f0, f1)) + int(not torch.equal(a0, a1))
        torch.cuda.synchronize()
        assert agg.poll() is None, 'the neighbour process ended before the measurement did'
    finally:
        agg.kill() if agg.poll() is None else None
        agg.wait()
    assert differing == 0
