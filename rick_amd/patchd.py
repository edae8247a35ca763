"""The two parts of CDC ("Few-shot Image Generation via Cross-domain Correspondence", Ojha et al., CVPR 2021) next to its
distance-consistency loss (rick_amd/cdc.py): the patch-level discriminator and the anchor-subspace sampling of the latents, on
the kernels of rick_amd/csrc/patchd.hip.

    heads = PatchHeads()                                     # one 3x3 conv to ONE channel + bias + LeakyReLU per tapped feature
    which, p_ind = draw_patch(i, subspace_freq, feat_ind)
    if which == 0:  z = sample_anchor_latents(anchors, batch, std);  pred, _ = d(g([z])[0])             # image-level, near an anchor
    else:           pred = patch_logits(d, heads, g(noise)[0], p_ind)                                    # [B, 1, h, w] patch logits

Neither the paper nor CDC's code was at hand.  The reference of this project still carries `get_subspace`
(train_dynamic_update_prune.py:148-156) and the flags --subspace_freq, --subspace_std, --feat_ind (:708-721); those parts are
restated from it.  The patch discriminator is RECALLED and unverified: CDC's `Extra` module as a list `new_conv` of
ConvLayer(512, 1, 3), applied to an intermediate feature of the discriminator chosen by `p_ind`, the discriminator's forward
ending there.  This docstring is the specification that is built.

Taps.  ``patch_taps(d)``: the indices into the feature list ``Discriminator.forward`` returns whose entries are a ResBlock's t1
(after conv1) or t2 (after conv2), have `channels` channels and a spatial size of 32 or 16, in list order; computed from the
module structure.  256 px, channel_multiplier 2: [6, 7, 8, 9] (b3.t2, b4.t1, b4.t2, b5.t1); 32 px: [1, 2, 3].

Patch forward.  ``patch_logits(d, heads, img, p_ind)``: d.convs[0], then the ResBlocks up to the one that owns tap
patch_taps(d)[p_ind]; a t1 tap runs only that block's conv1 (the rest of the block would be discarded, and in the one-node
form of the block it would cost full weight gradients of zeros), a t2 tap the whole block.  Then heads.new_conv[p_ind].
Nothing after the exit block runs; its parameters get no gradient (None, not zeros).  The losses are train.d_logistic_loss and
train.g_nonsaturating_loss over every entry of the map.

Head math (``patch_head``; x [N, C, H, W], w [1, C, 3, 3], b [1], wscale = 1 / sqrt(9 C), slope 0.2, gain sqrt(2)):

    z[n,y,x]    = b + sum_c sum_ky sum_kx (wscale w[c,ky,kx]) X[n,c,y+ky-1,x+kx-1]          (zero outside; correlation, as F.conv2d)
    out         = gain (z > 0 ? z : slope z)
    a           = gain (out > 0 ? 1 : slope)            (the sign of the stored output, as fused_act's backward takes it)
    gz = g a,   gb = sum gz
    gw[c,ky,kx] = wscale sum_{n,y,x} gz[n,y,x] X[n,c,y+ky-1,x+kx-1]
    gX[n,c,u,v] = wscale sum_{ky,kx} w[c,ky,kx] gz[n,u-ky+1,v-kx+1]

On the device, for fp32 tensors with C % 4 == 0, 4 <= C <= 2048 and fewer than 2^31 elements, this is rick_patch_head_fwd_f32
(one launch) and rick_patch_head_bwd_f32 + rick_patch_head_bwd_finish_f32 (``PatchHeadFn``, first order only): fixed summation
orders, bit-identical from run to run, and out[n] / gX[n] depend on image n alone (include/rick_hip.h "Patch head").  Other
device shapes, and every call under ``op.second_order_enabled()`` or ``use_kernels(False)``, take the composition of the
existing ops, op.conv2d + fused_leaky_relu, the bias added in between through fp64 (the same fp32 sum; its gradient is then an
fp64 sum over the map, as the kernels' is, where fused_leaky_relu's own bias gradient is an fp32 column sum that one channel of
512 values leaves 3.1e-6 from fp64).  Those ops refuse CPU tensors, so CPU tensors take the same definition from
torch.nn.functional (conv2d, leaky_relu), in the tensors' dtype.

Anchor sampling.  ``sample_anchor_latents`` restates get_subspace: rows drawn with numpy's randint, plus std * N(0, I).  The
reference draws element by element on the host (``z[i][j].data.normal_(z[i][j], std)``); here it is ONE torch.randn on the
anchors' device: the same distribution, not the same bits.

Schedule.  ``draw_patch(i, subspace_freq, feat_ind)``: which = i % subspace_freq; which == 0 is an anchor iteration (latents from
the anchor subspace, image-level discriminator in both steps); otherwise p_ind = randint(0, feat_ind) and both steps of the
iteration use the patch path at that tap, with random latents.

Deviation (train.RickTrainer): R1 stays on the image-level logits; CDC, as recalled, sends R1 through the patch head on patch
iterations.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import op

MAX_C = 2048             # rick_patch_head_*_f32
TAP_SIZES = (32, 16)
_KERNELS = True


def use_kernels(on=True):
    """Module switch: False forces ``patch_head`` onto the composition of the existing ops (benchmarks, tests).  Returns the
    previous setting."""
    global _KERNELS
    prev, _KERNELS = _KERNELS, bool(on)
    return prev


class PatchHeads(nn.Module):
    """CDC's `Extra`, recalled: ``new_conv``, `n_heads` ConvLayer(channels, 1, 3) with the initial values of the existing
    ConvLayer.  state_dict keys: new_conv.{i}.0.weight [1, channels, 3, 3], new_conv.{i}.1.bias [1]."""

    def __init__(self, n_heads=4, channels=512):
        super().__init__()
        from .models import ConvLayer
        self.channels = channels
        self.new_conv = nn.ModuleList(ConvLayer(channels, 1, 3) for _ in range(n_heads))

    def forward(self, x, p_ind):
        conv, act = self.new_conv[p_ind][0], self.new_conv[p_ind][1]
        return patch_head(x, conv.weight, act.bias, conv.scale, act.negative_slope, act.scale)


def _block_taps(d):
    """[(list index, block index in d.convs, 't1' | 't2', channels, spatial size)] of every ResBlock feature, from the modules."""
    blocks = list(d.convs)[1:]
    size = 2 ** (len(blocks) + 2)              # Discriminator: one ResBlock per halving, down to 4 px
    out = []
    for j, blk in enumerate(blocks):
        c1, c2 = blk.conv1[0], blk.conv2[-2]
        out.append((2 * j + 1, j + 1, 't1', c1.weight.shape[0], size // c1.stride))
        size //= c1.stride * c2.stride
        out.append((2 * j + 2, j + 1, 't2', c2.weight.shape[0], size))
    return out


def patch_taps(d, channels=512):
    """Indices into ``Discriminator.forward``'s feature list: the t1 / t2 entries with `channels` channels and spatial size 32 or
    16, in list order.  No forward pass."""
    return [i for i, _, _, c, s in _block_taps(d) if c == channels and s in TAP_SIZES]


def patch_logits(d, heads, img, p_ind):
    """[B, 1, h, w] patch logits of `img` at tap patch_taps(d)[p_ind] (module docstring, "Patch forward")."""
    taps = patch_taps(d, heads.channels)
    if not 0 <= p_ind < len(taps) or p_ind >= len(heads.new_conv):
        raise ValueError(f'patch_logits: p_ind {p_ind} with {len(taps)} taps and {len(heads.new_conv)} heads')
    _, exit_blk, which, _, _ = next(t for t in _block_taps(d) if t[0] == taps[p_ind])
    convs = list(d.convs)
    x = convs[0](img)
    for blk in convs[1:exit_blk]:
        x = blk(x)
    blk = convs[exit_blk]
    if which == 't1':
        tap = blk.conv1(x)
    else:
        feat = []
        blk(x, feat)
        tap = feat[1]
    return heads(tap, p_ind)


# ---- the head -----------------------------------------------------------------------------------------------------------------
def _eligible(x, w, b):
    if not (x.is_cuda and x.dtype == w.dtype == b.dtype == torch.float32 and w.device == x.device and b.device == x.device):
        return False
    if x.dim() != 4:
        return False
    N, C, H, W = x.shape
    return (C % 4 == 0 and 4 <= C <= MAX_C and min(N, H, W) >= 1 and x.numel() < 2 ** 31 and tuple(w.shape) == (1, C, 3, 3)
            and b.numel() == 1)


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.preserve_format)


class PatchHeadFn(torch.autograd.Function):
    """The head on rick_patch_head_fwd_f32 / rick_patch_head_bwd_f32 / rick_patch_head_bwd_finish_f32.  First order only:
    ``create_graph=True`` raises in the backward pass."""

    @staticmethod
    def forward(ctx, x, w, b, wscale, slope, gain):
        from . import _lib
        N, C, H, W = x.shape
        xd = _aligned(x.detach().contiguous(memory_format=torch.channels_last))
        wd, bd = _aligned(w.detach().contiguous()), b.detach().contiguous()
        out = torch.empty((N, 1, H, W), device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib.rick_patch_head_fwd_f32(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), out.data_ptr(), N, H, W, C,
                                                        wscale, slope, gain, _lib.stream_ptr()), 'rick_patch_head_fwd_f32')
        ctx.save_for_backward(xd, wd, out)
        ctx.cfg, ctx.b_shape = (wscale, slope, gain), tuple(b.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        if torch.is_grad_enabled():
            raise RuntimeError('patchd.patch_head: the backward pass is first order only (create_graph=True is not supported)')
        from . import _lib
        xd, wd, out = ctx.saved_tensors
        wscale, slope, gain = ctx.cfg
        N, C, H, W = xd.shape
        g = g.contiguous()
        gx = torch.empty_like(xd) if ctx.needs_input_grad[0] else None       # channels-last like xd: the gradient in x's layout
        gw, gb = torch.empty_like(wd), torch.empty(1, device=xd.device, dtype=torch.float32)
        with torch.cuda.device(xd.device):
            ws = torch.empty(_lib.lib.rick_patch_head_workspace_bytes(N, H, W, C) // 4, device=xd.device, dtype=torch.float32)
            _lib.check(_lib.lib.rick_patch_head_bwd_f32(xd.data_ptr(), wd.data_ptr(), g.data_ptr(), out.data_ptr(), _lib.ptr(gx),
                                                        ws.data_ptr(), N, H, W, C, wscale, slope, gain, _lib.stream_ptr()),
                       'rick_patch_head_bwd_f32')
            _lib.check(_lib.lib.rick_patch_head_bwd_finish_f32(ws.data_ptr(), gw.data_ptr(), gb.data_ptr(), N, H, W, C, wscale,
                                                               _lib.stream_ptr()), 'rick_patch_head_bwd_finish_f32')
        return (gx, gw if ctx.needs_input_grad[1] else None, gb.view(ctx.b_shape) if ctx.needs_input_grad[2] else None,
                None, None, None)


def _compose(x, w, b, wscale, slope, gain):
    """The head from the existing ops (device), or the same definition from torch.nn.functional (CPU tensors, any float dtype)."""
    if x.is_cuda:
        # The bias joins the one-channel map through fp64 (the rounded sum is the fp32 add's, bit for bit) so that its gradient,
        # the sum over the whole map, is accumulated in fp64 as the kernels accumulate it.  Handed to fused_leaky_relu, the bias
        # gradient would be that op's fp32 block-partial column sum: 3.1e-6 from fp64 over the 512 values of (2, 512, 16, 16),
        # 73 times the error of a CPU sum, because ONE channel carries the whole map.
        z = (op.conv2d(x, w, 1, 1, wscale).double() + b.double().view(1, -1, 1, 1)).to(x.dtype)
        return op.fused_leaky_relu(z, None, slope, gain)
    return F.leaky_relu(F.conv2d(x, w * wscale, padding=1) + b.view(1, -1, 1, 1), slope) * gain


def patch_head(x, w, b, wscale, slope=0.2, gain=2 ** 0.5):
    """gain * leaky_relu(conv2d(x, wscale * w, padding 1) + b, slope) for w [1, C, 3, 3], b [1] -> [N, 1, H, W].  Eligible device
    tensors run the kernels of rick_amd/csrc/patchd.hip; CPU tensors, ineligible shapes, second-order mode and
    ``use_kernels(False)`` take the composition."""
    if _KERNELS and not op.second_order_enabled() and _eligible(x, w, b):
        return PatchHeadFn.apply(x, w, b, float(wscale), float(slope), float(gain))
    return _compose(x, w, b, float(wscale), float(slope), float(gain))


# ---- anchors and schedule ------------------------------------------------------------------------------------------------------
def sample_anchor_latents(anchors, batch, std, rng=None, generator=None):
    """get_subspace (train_dynamic_update_prune.py:148-156): ``ind = randint(0, n, size=batch)`` from `rng` (a numpy RandomState)
    or numpy's global state, then anchors[ind] + std * N(0, I) — one torch.randn on the anchors' device (`generator`: its torch
    generator) where the reference draws element by element on the host: the same distribution, not the same bits.  std = 0
    returns anchors[ind] exactly."""
    if anchors.dim() != 2 or anchors.shape[0] < 1:
        raise ValueError(f'sample_anchor_latents: anchors must be [n >= 1, latent], got {tuple(anchors.shape)}')
    ind = (rng if rng is not None else np.random).randint(0, anchors.shape[0], size=batch)
    rows = anchors[torch.as_tensor(ind, dtype=torch.int64, device=anchors.device)]
    noise = torch.randn(batch, anchors.shape[1], device=anchors.device, dtype=anchors.dtype, generator=generator)
    return rows + std * noise


def draw_patch(i, subspace_freq, feat_ind, rng=None):
    """(which, p_ind) of iteration i: which = i % subspace_freq; (0, None) is an anchor iteration; otherwise p_ind =
    randint(0, feat_ind) from `rng` (a numpy RandomState) or numpy's global state."""
    which = i % subspace_freq
    if which == 0:
        return 0, None
    return which, int((rng if rng is not None else np.random).randint(0, feat_ind))
