"""Independent fp64 restatement of the VGG16 fc2 features behind the reference's improved precision / recall, written
from the five steps of gan_metrics/precision_recall.py:124-152 (IPR.extract_features) in plain torch CPU ops:

1. images [N, 3, H, W] in [-1, 1] as they are (no ImageNet affine);
2. F.interpolate(size=(224, 224)) (mode 'nearest') unless the images are 224 x 224 already;
3. torchvision vgg16.features: 13 conv3x3 + ReLU, five 2x2 max pools -> [N, 512, 7, 7];
4. .view(-1, 7 * 7 * 512): (c, y, x) order;
5. Linear(25088, 4096), ReLU, Linear(4096, 4096): the fc2 output before its ReLU.

Plus synthetic weights in torchvision's vgg16 state_dict layout, a smooth generator stand-in and the margin of a
precision / recall computation.  Nothing here imports rick_amd.vgg."""
import torch
import torch.nn.functional as F

from tests.lpips_f64 import CONVS, smooth_images  # noqa: F401  (re-exported)

POOL_AT = (4, 9, 16, 23, 30)


def synthetic_vgg16_state_dict(seed):
    """torchvision vgg16 layout.  Fan-in-scaled normals with the ReLU gain (std sqrt(2 / fan_in)) and small biases keep
    activations O(1) through all 15 layers."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for idx, ci, co in CONVS:
        sd[f'features.{idx}.weight'] = torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5
        sd[f'features.{idx}.bias'] = torch.randn(co, generator=g) * 0.02
    for idx, k in ((0, 25088), (3, 4096)):
        sd[f'classifier.{idx}.weight'] = torch.randn(4096, k, generator=g) * (2.0 / k) ** 0.5
        sd[f'classifier.{idx}.bias'] = torch.randn(4096, generator=g) * 0.02
    return sd


def fc2_f64(sd, x):
    """x [N, 3, H, W] fp32 -> fc2 features [N, 4096] in fp64."""
    if tuple(x.shape[2:]) != (224, 224):
        x = F.interpolate(x, size=(224, 224))                  # values are copied: resize in the input's dtype, as the reference
    h = x.double()
    weights = {idx: (sd[f'features.{idx}.weight'].double(), sd[f'features.{idx}.bias'].double()) for idx, _, _ in CONVS}
    for i in range(31):
        if i in weights:
            h = F.conv2d(h, weights[i][0], weights[i][1], 1, 1)
        elif i in POOL_AT:
            h = F.max_pool2d(h, 2, 2)
        else:
            h = torch.relu(h)
    assert tuple(h.shape[1:]) == (512, 7, 7)
    h = h.reshape(-1, 7 * 7 * 512)
    h = torch.relu(F.linear(h, sd['classifier.0.weight'].double(), sd['classifier.0.bias'].double()))
    return F.linear(h, sd['classifier.3.weight'].double(), sd['classifier.3.bias'].double())


def fc2_f64_batched(sd, x, step=8):
    return torch.cat([fc2_f64(sd, x[i:i + step]) for i in range(0, x.shape[0], step)])


class SmoothG(torch.nn.Module):
    """A generator stand-in: bilinear upsampling of tanh(z) seen as 3 x 4 x 4 (smooth, distinct images in [-0.9, 0.9])."""

    def __init__(self, size):
        super().__init__()
        self.size = size
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, zs):
        img = torch.tanh(zs[0][:, :48]).view(-1, 3, 4, 4)
        return F.interpolate(img, (self.size, self.size), mode='bilinear', align_corners=False) * 0.9, None


def pr_margin(fr, ff, k=3):
    """The smallest |distance - radius| / radius over every comparison improved precision / recall makes (a feature of one
    set against a ball of the other), in fp64.  A radius is itself a distance (the k-th neighbour's), so it moves no more than
    the features do: with every margin above 1e-4, fp32 features cannot flip a count."""
    fr, ff = fr.double(), ff.double()
    worst = float('inf')
    for ref, subj in ((fr, ff), (ff, fr)):
        radii = torch.cdist(ref, ref).kthvalue(k + 1, dim=1).values
        d = torch.cdist(ref, subj)
        worst = min(worst, float(((d - radii[:, None]).abs() / radii[:, None]).min()))
    return worst


def max_rel_err(got, ref):
    """max |got - ref| relative to the max-norm of ref."""
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())
