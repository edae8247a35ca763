"""Writes tests/golden/clip_text_tiny.npz from the locally installed `transformers` (nothing is downloaded); the tests read
only the .npz and never import transformers.

  python tools/make_clip_text_golden.py

1. A tiny CLIP text tower: CLIPTextModelWithProjection built from a config with seeded random weights (set as
   tools/make_clip_golden.py sets them: the library's init leaves biases 0 and LayerNorm at (1, 0)), its state_dict in the
   transformers layout as fp32 ('sd/...'), four id rows ('ids') and the fp64 `text_embeds` of the model run in .double() on them
   ('text_embeds').  Configuration: vocab 96, width 32, 2 layers, 2 heads, MLP 128, 12 positions, projection 16, hidden_act
   'quick_gelu', layer_norm_eps 1e-5, bos_token_id 94, eos_token_id 95.  The rows: a short prompt padded with 0, one padded
   with 95, one that fills all 12 positions, BOS then EOT alone.  tests/test_cliptext.py pins the fp64 restatement
   (tests/cliptext_f64.py) to these embeddings.
2. A tiny byte-level BPE vocabulary (the 256 byte symbols, their </w> forms, a dozen merges, the two specials), written to a
   temporary directory and loaded into the library's CLIPTokenizer; the vocabulary ('tok_vocab', JSON), the merges
   ('tok_merges', one pair per line), the test strings ('tok_texts', JSON), the context ('tok_context'), the library's pad id
   ('tok_pad_id') and its ids with truncation ('tok_ids').  'tok_long' lists the strings that are too long without truncation.

The file comes to about 125 KB, not a few tens: the prescribed model alone holds some 30 000 fp32 weights, which do not
compress, and the size is that of the other goldens (clip_tiny.npz: 168 KB)."""
import json
import os
import tempfile

os.environ['HF_HUB_OFFLINE'] = '1'
os.environ['TRANSFORMERS_OFFLINE'] = '1'

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'clip_text_tiny.npz')
CONFIG = dict(vocab_size=96, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=128,
              max_position_embeddings=12, projection_dim=16, hidden_act='quick_gelu', layer_norm_eps=1e-5, attention_dropout=0.0,
              bos_token_id=94, eos_token_id=95, pad_token_id=0)
IDS = [[94, 5, 17, 33, 95, 0, 0, 0, 0, 0, 0, 0],
       [94, 40, 2, 61, 7, 88, 95, 95, 95, 95, 95, 95],
       [94, 3, 93, 12, 12, 50, 71, 8, 29, 64, 1, 95],
       [94, 95, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]]
CONTEXT = 48
MERGES = [('t', 'h'), ('i', 'n'), ('th', 'e</w>'), ('a', 'n'), ('an', 'd</w>'), ('p', 'h'), ('o', 't'), ('ph', 'ot'), ('phot', 'o</w>'),
          ("'", 's</w>'), ('!', '!</w>'), ('d', 'o'), ('do', 'g</w>'), ('Ã', '©</w>'), ("'", 't</w>')]
TEXTS = ["The dog's photo isn't the dog",
         "I'm they've we'll; you're he'd 'tis",
         'in 2021, 42!!  ...and?! #9',
         '  leading   and\trepeated \n whitespace ',
         'Cafe\u0301 and caf\u00e9',                              # a decomposed accent that NFC composes, then the composed one
         '\u65e5\u672c \U0001f642 dog',                               # multi-byte characters
         'a dog <|endoftext|> the end',
         'THE DOG',
         'dog!<|endoftext|>the',                              # a special inside a punctuation run and against a letter
         'A <|ENDOFTEXT|> b <|startoftext|>?',                # only the exact spelling is the special
         'the dog and the photo ' * 10]                       # too long for the context


def byte_symbols():
    """GPT-2's printable byte table, in byte order."""
    keep = list(range(ord('!'), ord('~') + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    out, extra = [], 0
    for b in range(256):
        if b in keep:
            out.append(chr(b))
        else:
            out.append(chr(256 + extra))
            extra += 1
    return out


def model_golden():
    from transformers import CLIPTextConfig, CLIPTextModelWithProjection
    torch.manual_seed(20212)
    model = CLIPTextModelWithProjection(CLIPTextConfig(**CONFIG)).eval()
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
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
    ids = torch.tensor(IDS, dtype=torch.int64)
    with torch.no_grad():
        embeds = model.double()(input_ids=ids).text_embeds
    assert embeds.dtype == torch.float64 and tuple(embeds.shape) == (len(IDS), 16)
    arrays = {'sd/' + k: v.numpy() for k, v in sd.items()}
    arrays['ids'] = ids.numpy()
    arrays['text_embeds'] = embeds.numpy()
    return arrays, float(embeds.abs().max())


def tokenizer_golden():
    from transformers import CLIPTokenizer
    symbols = byte_symbols()
    names = symbols + [s + '</w>' for s in symbols] + [a + b for a, b in MERGES] + ['<|startoftext|>', '<|endoftext|>']
    assert len(set(names)) == len(names)
    vocab = {s: i for i, s in enumerate(names)}
    merges = '\n'.join(f'{a} {b}' for a, b in MERGES)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, 'vocab.json'), 'w', encoding='utf-8') as f:
            json.dump(vocab, f, ensure_ascii=False)
        with open(os.path.join(d, 'merges.txt'), 'w', encoding='utf-8') as f:
            f.write('#version: 0.2\n' + merges + '\n')
        tok = CLIPTokenizer.from_pretrained(d)
    rows = tok(TEXTS, padding='max_length', max_length=CONTEXT, truncation=True)['input_ids']
    free = tok(TEXTS)['input_ids']
    long = [i for i, r in enumerate(free) if len(r) > CONTEXT]
    assert long == [len(TEXTS) - 1], long
    return {'tok_vocab': np.array(json.dumps(vocab, ensure_ascii=False)), 'tok_merges': np.array(merges),
            'tok_texts': np.array(json.dumps(TEXTS, ensure_ascii=False)), 'tok_context': np.array(CONTEXT),
            'tok_pad_id': np.array(tok.pad_token_id), 'tok_ids': np.array(rows, dtype=np.int64), 'tok_long': np.array(long, dtype=np.int64)}


def main():
    arrays, top = model_golden()
    arrays.update(tokenizer_golden())
    np.savez_compressed(OUT, **arrays)
    print(f'wrote {OUT}: {os.path.getsize(OUT)} bytes, |embeds|max {top:.3f}')
    print(arrays['tok_ids'])


if __name__ == '__main__':
    main()
