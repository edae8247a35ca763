"""rick_amd/param_block.py on its own, without either augmentation recipe or a kernel: the persistent parameter block of a training
step (byte order, address, back-to-back refills, the size check) and the closed pair of autograd functions."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REC = np.dtype([('f', '<f4', 4), ('i', '<i4', 6)])          # a 40-byte record
assert REC.itemsize == 40


def _calls(seed):
    """Two calls of two records each, every byte drawn from the seed."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, 2 * REC.itemsize, dtype=np.uint8).view(REC) for _ in range(2)]


def test_step_block_orders_bytes_keeps_its_address_and_survives_back_to_back_refills():
    from rick_amd.param_block import StepParamBlock
    blk = StepParamBlock(REC.itemsize, 2 * 2, 'cuda', who='stepname')
    assert blk.dev.dtype == torch.uint8 and blk.dev.numel() == 160 and blk.dev.is_cuda and not bool(blk.dev.any())
    addr = blk.dev.data_ptr()
    c0, c1 = _calls(1)
    assert blk.fill([c0, c1], reverse=True) is blk
    assert blk.dev.cpu().numpy().tobytes() == c1.tobytes() + c0.tobytes()
    assert blk.calls[0] is c0 and blk.calls[1] is c1                    # draw order, whatever the launch's order
    blk.fill([c0, c1], reverse=False)
    assert blk.dev.cpu().numpy().tobytes() == c0.tobytes() + c1.tobytes()
    assert blk.calls[0] is c0 and blk.calls[1] is c1
    # three refills with no host synchronisation between them: each is on the device when the stream reaches it (the clone is
    # ordered behind its copy), so no refill overwrote a staging buffer whose copy was still in flight, and the third one stays
    torch.cuda.synchronize()
    fills = [_calls(10 + k) for k in range(3)]
    snaps = [blk.fill(calls, reverse=True).dev.clone() for calls in fills]
    for calls, snap in zip(fills, snaps):
        assert snap.cpu().numpy().tobytes() == calls[1].tobytes() + calls[0].tobytes()
    assert blk.dev.cpu().numpy().tobytes() == fills[2][1].tobytes() + fills[2][0].tobytes()
    assert blk.calls[0] is fills[2][0] and blk.calls[1] is fills[2][1]
    assert blk.dev.data_ptr() == addr
    with pytest.raises(RuntimeError, match='stepname: parameter block of 200 bytes does not fit 160'):
        blk.fill([c0, c1, c0[:1]])
    assert blk.dev.data_ptr() == addr


def test_linear_pair_is_closed_under_differentiation():
    """y = 2 x + offset with adjoint 2 g, written in torch: the gradient through Fn is AdjFn's result, the double backward is the
    offset-free forward, the parameters receive no gradient."""
    from rick_amd.param_block import linear_pair
    log = []

    def launch(entry, x, params, bias):
        log.append((entry, bias))
        return 2 * x + params.sum() if entry == 'fwd' and bias else 2 * x

    Fn, AdjFn = linear_pair(launch, 'ToyFn', 'ToyAdjFn')
    assert (Fn.__name__, AdjFn.__name__) == ('ToyFn', 'ToyAdjFn')
    gen = torch.Generator().manual_seed(3)
    x, gy, v = (torch.randn(2, 3, 4, 4, generator=gen).cuda().requires_grad_(True) for _ in range(3))
    params = torch.tensor([0.25, 0.5], device='cuda', requires_grad=True)
    y = Fn.apply(x, params)
    assert torch.equal(y, 2 * x + 0.75) and log == [('fwd', True)]
    gx, gp = torch.autograd.grad(y, [x, params], gy, create_graph=True, allow_unused=True)
    assert gp is None
    assert torch.equal(gx, AdjFn.apply(gy, params)) and torch.equal(gx, 2 * gy) and log[1] == ('adj', False)
    del log[:]
    (ggy,) = torch.autograd.grad(gx, gy, v, create_graph=True)          # the backward of the adjoint: Fn without the offset
    assert log == [('fwd', False)]
    assert torch.equal(ggy, Fn.apply(v, params, False)) and torch.equal(ggy, 2 * v)
    (gv,) = torch.autograd.grad(ggy, v, gy)                             # and once more: the adjoint again
    assert log[-1] == ('adj', False) and torch.equal(gv, 2 * gy)
