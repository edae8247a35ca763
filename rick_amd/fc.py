"""What the users of rick_fc_f32 (include/rick_hip.h) share: the VGG16 fc2 features (rick_amd/vgg.py) and the InceptionV3
classifier head (rick_amd/inception.py)."""
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
