"""Writes tests/golden/clip_tiny.npz: a tiny CLIP image tower from the locally installed `transformers`
(CLIPVisionModelWithProjection built from a config with seeded random weights: nothing is downloaded), its state_dict in the
transformers layout as fp32, three fp32 images in [-1, 1] already at the model's 32 x 32, and the fp64 `image_embeds` of the model run in
.double() on those fp32 weights and on CLIP's affine of the images (formed in fp64).  tests/test_clip.py pins the fp64 restatement (tests/clip_f64.py) to these embeddings; the
tests read only the .npz and never import transformers.

  python tools/make_clip_golden.py

Configuration: width 32, 2 layers, 2 heads, MLP 128, patch 8, image 32, projection 16, hidden_act 'quick_gelu',
layer_norm_eps 1e-5 (CLIP's own)."""
import os

os.environ['HF_HUB_OFFLINE'] = '1'
os.environ['TRANSFORMERS_OFFLINE'] = '1'

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'clip_tiny.npz')
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
CONFIG = dict(hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128, patch_size=8, image_size=32,
              projection_dim=16, hidden_act='quick_gelu', layer_norm_eps=1e-5, attention_dropout=0.0)


def main():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(20211)
    model = CLIPVisionModelWithProjection(CLIPVisionConfig(**CONFIG)).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():                                     # the library's init leaves biases 0 and LayerNorm at (1, 0)
        for name, p in model.named_parameters():
            if name.endswith('bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif 'norm' in name and name.endswith('weight'):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() >= 2 and 'embedding' not in name:
                p.copy_(torch.randn(p.shape, generator=g) * p[0].numel() ** -0.5)
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    sd = {k: v.detach().float().contiguous() for k, v in model.state_dict().items() if not k.endswith('position_ids')}
    images = (torch.rand(3, 3, 32, 32, generator=g) * 2 - 1).float()       # in [-1, 1], already at the model's size
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (MEAN, STD))
    with torch.no_grad():                                     # CLIP's affine in fp64; no resize at 32 x 32
        embeds = model.double()(pixel_values=(images.double() * 0.5 + 0.5 - mean) / std).image_embeds
    assert embeds.dtype == torch.float64 and tuple(embeds.shape) == (3, 16)
    arrays = {'sd/' + k: v.numpy() for k, v in sd.items()}
    arrays['images'] = images.numpy()
    arrays['image_embeds'] = embeds.numpy()
    np.savez_compressed(OUT, **arrays)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(sd)} tensors, |embeds|max {float(embeds.abs().max()):.3f}')


if __name__ == '__main__':
    main()
