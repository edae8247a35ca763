"""What tests/test_gpu_gemm_forms.py holds the f32 GEMM convolution (rick_inc_conv_f32, rick_inc_conv_bwd_f32,
rick_inc_conv_lin_f32) and the fully connected layer (rick_fc_f32) to: the fp64 expressions of include/rick_hip.h written out
with F.conv2d / F.conv_transpose2d / F.linear on NCHW tensors, the packed operand layouts restated index by index
(independently of rick_amd.gemm_conv.pack, pack_transposed and rick_amd/fc.py), and the host side of the launchers replayed:
the column block, the kernel instantiation, fc_plan.  A plain module: no fixtures, no pytest hooks; everything runs on the CPU."""
import torch
import torch.nn.functional as F


def cdiv(a, b):
    return -(-a // b)


def out_hw(h, w, k, s, p):
    return (h + 2 * p[0] - k[0]) // s[0] + 1, (w + 2 * p[1] - k[1]) // s[1] + 1


# ------------------------------------------------------------------------------------------------------ packed layouts
def pack_wpk(w, bn, bias=None):
    """w [Co, Ci, kh, kw] -> wpk [Kp, Cop] fp32, wpk[(ky * kw + kx) * Ci + ci][co] = w[co][ci][ky][kx]; K rounded up to 32 rows, Co
    to bn columns, the padding zero; and the bias [Cop]."""
    co, ci, kh, kw = w.shape
    K = kh * kw * ci
    wpk = torch.zeros(cdiv(K, 32) * 32, cdiv(co, bn) * bn, dtype=torch.float32)
    for ky in range(kh):
        for kx in range(kw):
            row = (ky * kw + kx) * ci
            wpk[row:row + ci, :co] = w[:, :, ky, kx].t()
    bp = torch.zeros(wpk.shape[1], dtype=torch.float32)
    if bias is not None:
        bp[:co] = bias
    return wpk, bp


def pack_wt(w, bn):
    """The forward filter w [Cf, Cin, 3, 3] -> the data gradient's operand wt [Kp, Cop], rows (ky, kx, cf), columns cin:
    wt[(ky * 3 + kx) * Cf + cf][cin] = w[cf][cin][2 - ky][2 - kx]."""
    cf, cin, kh, kw = w.shape
    wt = torch.zeros(cdiv(kh * kw * cf, 32) * 32, cdiv(cin, bn) * bn, dtype=torch.float32)
    for ky in range(kh):
        for kx in range(kw):
            row = (ky * kw + kx) * cf
            wt[row:row + cf, :cin] = w[:, :, kh - 1 - ky, kw - 1 - kx]
    return wt


def pack_fc(w):
    """W [N, K] -> [Np / 32][Kp / 8][64 lanes][4] flat, Np = N rounded up to 128, Kp = K up to 8, zero padded: lane (h = lane >> 5,
    c = lane & 31) of column block nb and k block kb holds W[32 nb + c][8 kb + 2 j + h] in component j."""
    n, k = w.shape
    np_, kp = cdiv(n, 128) * 128, cdiv(k, 8) * 8
    wp = torch.zeros(np_, kp, dtype=torch.float32)
    wp[:n, :k] = w
    nb, kb = torch.arange(np_ // 32).view(-1, 1, 1, 1), torch.arange(kp // 8).view(1, -1, 1, 1)
    lane, j = torch.arange(64).view(1, 1, -1, 1), torch.arange(4).view(1, 1, 1, -1)
    return wp[32 * nb + (lane & 31), 8 * kb + 2 * j + (lane >> 5)].reshape(-1)


# ------------------------------------------------------------------------------------------------------ fp64 expressions
def _nchw(x):
    return x.double().permute(0, 3, 1, 2)


def _rows(y):
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


def quickgelu_f64(u):
    return u / (1 + torch.exp(-1.702 * u))


def conv_f64(x, w, bias, s, p):
    """x [N, H, W, Ci] NHWC, w [Co, Ci, kh, kw] -> conv(x, w) + bias as rows [M, Co], fp64."""
    return _rows(F.conv2d(_nchw(x), w.double(), None if bias is None else bias.double(), stride=s, padding=p))


def conv_fwd_f64(x, w, bias, s, p):
    return conv_f64(x, w, bias, s, p).clamp_min(0)


def conv_lin_f64(x, w, bias, s, p, act, res):
    v = conv_f64(x, w, bias, s, p)
    if act:
        v = quickgelu_f64(v)
    return v if res is None else v + res.double()


def conv_lin_f32(x, w, bias, s, p, act, res):
    """The fp32 torch-CPU composition the QuickGELU bases are measured with (never the kernel)."""
    v = _rows(F.conv2d(x.permute(0, 3, 1, 2), w, bias, stride=s, padding=p))
    if act:
        v = v * torch.sigmoid(1.702 * v)
    return v if res is None else v + res


def conv_bwd_f64(gout, w, mask, add):
    """gout [N, H, W, Cf], the forward filter w [Cf, Cin, 3, 3] (stride 1, pad 1) -> rows [M, Cin]:
    (mask > 0) ? conv_transpose(gout, w) + add : 0."""
    v = _rows(F.conv_transpose2d(_nchw(gout), w.double(), padding=1))
    if add is not None:
        v = v + add.double()
    return v if mask is None else torch.where(mask > 0, v, torch.zeros_like(v))


def fc_f64(x, w, bias, relu):
    v = F.linear(x.double(), w.double(), bias.double())
    return v.clamp_min(0) if relu else v


# -------------------------------------------------------------------------------------------------- the launchers, replayed
def column_block(co):
    """rick_amd.gemm_conv.column_block: the block of 64 or 128 columns that pads co least, 128 on a tie."""
    return 128 if cdiv(co, 128) * 128 <= cdiv(co, 64) * 64 else 64


def conv_form(kind, bn, act=0):
    """The instantiation of inc_conv_kernel<NT, BWD, LIN> a launch takes: NT = bn / 64; rick_inc_conv_lin_f32 picks LIN = 2 with
    act and LIN = 1 without; the residual is a run-time pointer."""
    assert bn in (64, 128)
    arm = {'fwd': 'fwd', 'bwd': 'bwd', 'lin': f'lin{2 if act else 1}'}[kind]
    return f'conv<NT{bn // 64},{arm}>'


CONV_FORMS = [f'conv<NT{nt},{arm}>' for nt in (1, 2) for arm in ('fwd', 'bwd', 'lin1', 'lin2')]

FC_KB, FC_BN, FC_CH, FC_TARGET_BLOCKS, FC_MIN_SLICE_KB = 8, 128, 8, 512, 32


def fc_plan(K, N):
    """fc_plan of vgg.hip: (slices, k blocks per slice), a function of (K, N) only."""
    KB, nbk = cdiv(K, FC_KB), cdiv(N, FC_BN)
    S = max(1, min(cdiv(FC_TARGET_BLOCKS, nbk), KB // FC_MIN_SLICE_KB))
    kbs = cdiv(KB, S)
    return cdiv(KB, kbs), kbs


def fc_form(M, K, x_off):
    """fc_partial_kernel<MT> and its staging: MT = 1 up to 32 rows, vec when K % 4 == 0 and x is 16-byte aligned (x_off: floats
    of misalignment)."""
    return f"fc<MT{1 if M <= 32 else 2},{'vec' if K % 4 == 0 and x_off % 4 == 0 else 'scalar'}>"


FC_FORMS = [f'fc<MT{mt},{v}>' for mt in (1, 2) for v in ('vec', 'scalar')]


def fc_packed_floats(K, N):
    return cdiv(N, FC_BN) * FC_BN * cdiv(K, FC_KB) * FC_KB


def fc_workspace_floats(M, K, N):
    return fc_plan(K, N)[0] * M * N
