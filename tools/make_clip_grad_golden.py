"""Writes tests/golden/clip_tiny_grad.npz: the gradient of the tiny CLIP image tower of tests/golden/clip_tiny.npz with respect
to its images, from the locally installed `transformers` (CLIPVisionModelWithProjection rebuilt from the golden's own fp32
weights, run in .double(): nothing is downloaded).  It holds r [3, 16] fp64 (seeded) and d sum(image_embeds * r) / d images
[3, 3, 32, 32] fp64, the images entering through CLIP's affine formed in fp64, as in tools/make_clip_golden.py.
tests/test_clip_grad.py pins torch autograd of the fp64 restatement (tests/clip_f64.embed_f64) to it; the tests read only the
.npz files and never import transformers.

  python tools/make_clip_grad_golden.py"""
import os

os.environ['HF_HUB_OFFLINE'] = '1'
os.environ['TRANSFORMERS_OFFLINE'] = '1'

import numpy as np  # noqa: E402
import torch  # noqa: E402

from make_clip_golden import CONFIG, MEAN, STD, OUT as FORWARD  # noqa: E402

OUT = os.path.join(os.path.dirname(FORWARD), 'clip_tiny_grad.npz')


def main():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    z = np.load(FORWARD)
    model = CLIPVisionModelWithProjection(CLIPVisionConfig(**CONFIG)).eval()
    missing, unexpected = model.load_state_dict({k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}, strict=False)
    assert not unexpected and all(k.endswith('position_ids') for k in missing), (missing, unexpected)
    model = model.double()
    images = torch.from_numpy(z['images']).double().requires_grad_()
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (MEAN, STD))
    embeds = model(pixel_values=(images * 0.5 + 0.5 - mean) / std).image_embeds
    assert float((embeds.detach() - torch.from_numpy(z['image_embeds'])).abs().max()) < 1e-12      # the forward golden's model
    r = torch.randn(embeds.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(17))
    (grad,) = torch.autograd.grad((embeds * r).sum(), images)
    np.savez_compressed(OUT, r=r.numpy(), grad=grad.numpy())
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes, |grad|max {float(grad.abs().max()):.4f}')


if __name__ == '__main__':
    main()
