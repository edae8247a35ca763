"""What the per-image-parameter augmentations (rick_amd/augment.py, rick_amd/diffaug.py) share: the host records of a launch go to
the device as one uint8 parameter block — pinned, double-buffered staging into a persistent tensor that captured step graphs read —
and the fused op on such a block is a closed pair of autograd functions, each the other's backward."""
import numpy as np
import torch
from torch.autograd import Function


class ParamStaging:
    """Pinned, double-buffered host staging for parameter blocks: a buffer is refilled only after the copy that last read it
    has completed (its event), so an in-flight host-to-device copy is never overwritten."""

    def __init__(self):
        self.bufs, self.events, self.k = [None, None], [None, None], 0

    def upload(self, block, dst):
        raw = block.view(np.uint8).reshape(-1)
        k = self.k = 1 - self.k
        if self.events[k] is not None:
            self.events[k].synchronize()
        if self.bufs[k] is None or self.bufs[k].numel() < raw.size:
            self.bufs[k] = torch.empty(max(raw.size, 4096), dtype=torch.uint8, pin_memory=True)
        buf = self.bufs[k][:raw.size]
        buf.numpy()[:] = raw
        dst.view(-1)[:raw.size].copy_(buf, non_blocking=True)
        ev = self.events[k] = torch.cuda.Event()
        ev.record()
        return dst


_staging = ParamStaging()


def upload_params(block, device, dst=None, staging=None, who='upload_params'):
    """Copy a parameter block to the device: into `dst` (a persistent uint8 tensor that captured graphs read) or a new tensor.
    `who` names the caller in the error for a block that does not fit `dst`."""
    if dst is None:
        dst = torch.empty(block.nbytes, dtype=torch.uint8, device=device)
    elif dst.numel() < block.nbytes:
        raise RuntimeError(f'{who}: parameter block of {block.nbytes} bytes does not fit {dst.numel()}')
    return (staging or _staging).upload(block, dst)


class StepParamBlock:
    """The parameter block of one training step: `dev`, a zero-initialised uint8 device tensor for `n` records of `itemsize` bytes
    that keeps its address for the life of the object (captured graphs read it), its own staging, and `calls`, the host blocks of
    the last fill in draw order.  Create it outside a capture (the step's first, eager call)."""

    def __init__(self, itemsize, n, device, who='StepParamBlock'):
        self.dev = torch.zeros(n * itemsize, dtype=torch.uint8, device=device)
        self.staging, self.calls, self.who = ParamStaging(), [], who

    def fill(self, blocks, reverse=False):
        """Upload the per-call host blocks as one block; `reverse`: the launch's images are in the opposite order of the draws."""
        upload_params(np.concatenate(blocks[::-1] if reverse else blocks), self.dev.device, dst=self.dev, staging=self.staging,
                      who=self.who)
        self.calls = blocks
        return self


def linear_pair(launch, name, adj_name):
    """The autograd functions (Fn, AdjFn) of an op that is linear in x up to an offset, from `launch(entry, x, params, bias)`:
    entry 'fwd' evaluates the map (`bias`: with the offset), 'adj' the adjoint of its linear part.  Fn.apply(x, params, bias=True);
    its backward is AdjFn.apply(gy, params), whose backward is Fn without the offset — closed under differentiation to any order.
    No gradient flows to the parameters."""

    def fwd(ctx, x, params, bias=True):
        ctx.save_for_backward(params)
        return launch('fwd', x, params, bias)

    def fwd_backward(ctx, gy):
        (params,) = ctx.saved_tensors
        return adj_fn.apply(gy, params), None, None

    def adj(ctx, gy, params):
        ctx.save_for_backward(params)
        return launch('adj', gy, params, False)

    def adj_backward(ctx, gg):
        (params,) = ctx.saved_tensors
        return fn.apply(gg, params, False), None

    fn = type(name, (Function,), {'forward': staticmethod(fwd), 'backward': staticmethod(fwd_backward),
                                  '__doc__': f'y = op(x) for fixed per-image parameters; backward: {adj_name} (linear_pair).'})
    adj_fn = type(adj_name, (Function,), {'forward': staticmethod(adj), 'backward': staticmethod(adj_backward),
                                          '__doc__': f'gx = (linear part of {name})^T gy (linear_pair).'})
    return fn, adj_fn


def fused_launch(who, itemsize, entry_prefix, workspace):
    """The `launch(entry, x, params, bias)` of a fused HIP op on CUDA float32 [N, 3, H, W] images and a device block of N records of
    `itemsize` bytes: the library's `<entry_prefix>_fwd_f32` / `<entry_prefix>_adj_f32` with the workspace tensor that
    `workspace(lib, n, h, w, device)` returns (it raises for a shape the kernels do not take)."""
    fwd, adj = f'{entry_prefix}_fwd_f32', f'{entry_prefix}_adj_f32'

    def launch(entry, x, params, bias):
        from ._lib import check, lib, ptr, require_cuda_f32, stream_ptr
        require_cuda_f32(x)
        x = x.contiguous()
        n, c, h, w = x.shape
        nbytes = params.numel() * params.element_size()
        if c != 3 or not params.is_cuda or nbytes < n * itemsize:
            raise RuntimeError(f'{who}: needs [N, 3, H, W] images and N parameter entries on the device; got {tuple(x.shape)}, '
                               f'{nbytes} bytes')
        ws = workspace(lib, n, h, w, x.device)
        y = torch.empty_like(x)
        if entry == 'fwd':
            check(getattr(lib, fwd)(ptr(x), ptr(params), ptr(ws), ptr(y), n, h, w, int(bias), stream_ptr()), fwd)
        else:
            check(getattr(lib, adj)(ptr(x), ptr(params), ptr(ws), ptr(y), n, h, w, stream_ptr()), adj)
        return y
    return launch
