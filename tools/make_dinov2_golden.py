"""Writes tests/golden/dinov2_tiny.npz: a tiny DINOv2 ViT from the locally installed `transformers` (Dinov2Model built from a
config with seeded random weights: nothing is downloaded), its state_dict in the transformers layout as fp32, three fp32 images
in [-1, 1] at the model's 56 x 56 and the same three at 42 x 42, and for both sizes the fp64 `pooler_output` (the final
LayerNorm's class token) of the model run in .double() on those fp32 weights and on ImageNet's affine of the images (formed in
fp64).  At 42 x 42 the model interpolates its 4 x 4 positional grid to 3 x 3 (Dinov2Embeddings.interpolate_pos_encoding; that
one step runs in fp32 inside the library, whatever the model's dtype).  tests/test_dinov2.py pins the fp64 restatement
(tests/dinov2_f64.py) to these outputs; the tests read only the .npz and never import transformers.

  python tools/make_dinov2_golden.py

Configuration: hidden 32, 2 layers, 2 heads, mlp_ratio 4, patch 14, image 56, hidden_act 'gelu', layer_norm_eps 1e-6."""
import os

os.environ['HF_HUB_OFFLINE'] = '1'
os.environ['TRANSFORMERS_OFFLINE'] = '1'

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'dinov2_tiny.npz')
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
CONFIG = dict(hidden_size=32, num_hidden_layers=2, num_attention_heads=2, mlp_ratio=4, patch_size=14, image_size=56, hidden_act='gelu',
              layer_norm_eps=1e-6, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0, use_swiglu_ffn=False)


def main():
    from transformers import Dinov2Config, Dinov2Model
    torch.manual_seed(20230414)
    model = Dinov2Model(Dinov2Config(**CONFIG)).eval()
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():                                     # the library's init leaves biases 0, LayerNorm at (1, 0), lambda1 at 1
        for name, p in model.named_parameters():
            if name.endswith('bias'):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif name.endswith('lambda1'):
                p.copy_(0.5 + 0.5 * torch.rand(p.shape, generator=g))
            elif 'norm' in name and name.endswith('weight'):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 2 or p.dim() == 4:
                p.copy_(torch.randn(p.shape, generator=g) * p[0].numel() ** -0.5)
            else:                                             # cls_token, position_embeddings, mask_token
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
    sd = {k: v.detach().float().contiguous() for k, v in model.state_dict().items()}
    images = {s: (torch.rand(3, 3, s, s, generator=g) * 2 - 1).float() for s in (56, 42)}      # in [-1, 1]; no resize at either size
    mean, std = (torch.tensor(v, dtype=torch.float64).view(1, 3, 1, 1) for v in (MEAN, STD))
    model = model.double()
    arrays = {'sd/' + k: v.numpy() for k, v in sd.items()}
    for s, x in images.items():
        with torch.no_grad():                                 # ImageNet's affine in fp64
            pooled = model(pixel_values=(x.double() * 0.5 + 0.5 - mean) / std).pooler_output
        assert pooled.dtype == torch.float64 and tuple(pooled.shape) == (3, 32)
        arrays[f'images_{s}'], arrays[f'pooler_output_{s}'] = x.numpy(), pooled.numpy()
    np.savez_compressed(OUT, **arrays)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(sd)} tensors, ' +
          ', '.join(f'|pooler_output_{s}|max {float(np.abs(arrays[f"pooler_output_{s}"]).max()):.3f}' for s in images))


if __name__ == '__main__':
    main()
