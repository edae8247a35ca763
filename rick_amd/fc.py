"""What the users of rick_fc_f32 (include/rick_hip.h) share: the VGG16 fc2 features (rick_amd/vgg.py) and the InceptionV3
classifier head (rick_amd/inception.py).  The weight layout, its size check against the library and the chunked launch."""
import torch.nn.functional as F

FC_MAX_ROWS = 64                # rick_fc_f32 takes 1 <= M <= 64 rows per call


def pack_fc_weight(w):
    """W [N, K] fp32 -> the layout rick_fc_f32 streams (include/rick_hip.h): [Np / 32][Kp / 8][64 lanes][4], zero padded to
    Np = N rounded up to 128 and Kp = K rounded up to 8; lane (h = lane >> 5, c = lane & 31) of column block nb and k block kb
    holds W[32 nb + c][8 kb + 2 j + h] in component j."""
    n, k = w.shape
    np_, kp = -(-n // 128) * 128, -(-k // 8) * 8
    wp = F.pad(w, (0, kp - k, 0, np_ - n))
    return wp.view(np_ // 32, 32, kp // 8, 4, 2).permute(0, 2, 4, 1, 3).contiguous().view(-1)       # (nb, kb, h, c, j)


def check_packed(wpk, k, n, who):
    """The packed weight of a [n, k] layer must have the size the kernel expects."""
    from . import _lib
    want = _lib.lib.rick_fc_packed_floats(k, n)
    if wpk.numel() != want:
        raise RuntimeError(f'{who}: packed fc weight has {wpk.numel()} floats, the kernel expects {want}')


def run_fc(src, wpk, bias, ws, dst, m, k, n, relu):
    """Rows [0, m) of src [m, k] through the layer -> dst [m, n], in chunks of FC_MAX_ROWS rows on the current stream.  src,
    wpk, bias, dst: pointers; ws: rick_fc_workspace_floats(min(m, FC_MAX_ROWS), k, n) floats."""
    from . import _lib as lib
    for lo in range(0, m, FC_MAX_ROWS):
        lib.check(lib.lib.rick_fc_f32(src + 4 * lo * k, wpk, bias, ws, dst + 4 * lo * n, min(FC_MAX_ROWS, m - lo), k, n, relu,
                                      lib.stream_ptr()), 'rick_fc_f32')
