"""What the evaluation networks (rick_amd/inception.py, vgg.py, lpips.py) and the two CLIP towers (clip.py, cliptext.py, through
cliptower.py) share around their kernels: reading a state_dict, checking an image batch, naming the device.  `who` is the
class the error message names."""
import torch


def load_dict(src):
    """src: a state_dict, or a path to one (torch.load, weights_only)."""
    if isinstance(src, dict):
        return src
    return torch.load(src, map_location='cpu', weights_only=True)


def get(sd, key, shape, who, errors=(KeyError, ValueError), dtype=torch.float32):
    """sd[key] as a contiguous CPU tensor of `dtype`; errors = (missing key, wrong shape), either names the key."""
    if key not in sd:
        raise errors[0](f'{who}: missing key {key!r}')
    v = torch.as_tensor(sd[key])
    if tuple(v.shape) != tuple(shape):
        raise errors[1](f'{who}: key {key!r} has shape {tuple(v.shape)}, expected {tuple(shape)}')
    return v.detach().to('cpu', dtype).contiguous()


def cuda_device(device):
    """torch.device(device); a 'cuda' without an index becomes the current device."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return device


def check_images(x, who, device, what='images', dtypes=(torch.float32,), min_size=None, noun='network'):
    """x must be [N, 3, H, W] of one of `dtypes`, H and W at least min_size, on the CPU or on `device`."""
    if x.dim() != 4 or x.shape[1] != 3:
        raise RuntimeError(f'{who}: expected {what} [N, 3, H, W], got {tuple(x.shape)}')
    if x.dtype not in dtypes:
        raise RuntimeError(f'{who}: {what} must be {" or ".join(str(d)[6:] for d in dtypes)}, got {x.dtype}')
    if min_size is not None and min(x.shape[2:]) < min_size:
        raise ValueError(f'{who}: images must be at least {min_size} x {min_size}, got {tuple(x.shape[2:])}')
    if x.device.type != 'cpu' and x.device != device:
        raise RuntimeError(f'{who}: {what} on {x.device}, {noun} loaded for {device}')
