"""CPU: the CLIP text tower's host side (rick_amd/cliptext.py, rick_amd/cliptok.py, clipguide.text_direction): the fp64
restatement (tests/cliptext_f64.py) pinned to the golden embeddings of an implementation the author did not write, the loader
in both layouts, a whole-model checkpoint in both towers, every refusal, the fp32 torch composition against the restatement,
the EOT rule, the tokenizer against the golden id rows of that implementation's tokenizer, and the text direction.

Tolerances of the fp32 composition: its own error against the fp64 restatement, measured once here and written down below
(max error over the reference's max-norm), x 4 for another BLAS or thread count."""
import json
import os

import numpy as np
import pytest
import torch

from tests.clip_f64 import synthetic_clip_state_dict
from tests.cliptext_f64 import direction_f64, first_max, max_rel_err, synthetic_text_state_dict, text_embed_f64, text_prompts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clip_text_tiny.npz')
CFG = dict(width=64, tokens=16, vocab=96, layers=2, mlp=256, dim=32)          # 4 heads of 16
HEADS = 4
TOK_CFG = dict(width=32, tokens=48, vocab=529, layers=1, mlp=64, dim=16)      # the golden tokenizer's context and vocabulary
TOK_HEADS = 2
IMAGE_CFG = dict(width=64, patch=8, image=32, layers=2, mlp=256, dim=32)
FACTOR = 4
# ClipTextFeatures on CPU ids against the fp64 restatement: CFG with seed 11 on text_prompts(n, 16, 96, seed=n), and the golden
NET_CPU_BASE = {3: 3.985e-07, 9: 3.957e-07}
GOLDEN_CPU_BASE = 4.510e-07
# text_direction on the CPU path against direction_f64 of the restatement's embeddings: TOK_CFG with seed 5, 'dog' -> 'photo',
# TEMPLATES
DIRECTION_CPU_BASE = 9.556e-07
TEMPLATES = ('a photo of a {}.', 'the {}!', '{}')


def golden():
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    return sd, torch.from_numpy(z['ids']), torch.from_numpy(z['text_embeds'])


def golden_tokenizer(**kw):
    from rick_amd.cliptok import ClipTokenizer
    z = np.load(GOLDEN)
    merges = [tuple(line.split(' ')) for line in str(z['tok_merges']).split('\n')]
    kw.setdefault('context', int(z['tok_context']))
    return ClipTokenizer(json.loads(str(z['tok_vocab'])), merges, **kw), z


def load(sd, **kw):
    from rick_amd.cliptext import ClipTextFeatures
    return ClipTextFeatures.load(sd, device='cpu', **kw)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_embeddings():
    sd, ids, ref = golden()
    assert ref.dtype == torch.float64 and ids.dtype == torch.int64 and all(v.dtype == torch.float32 for v in sd.values())
    assert tuple(ids.shape) == (4, 12) and ids[0, -1] == 0 and ids[1, -1] == 95 and ids[2, -1] == 95 and ids[3].tolist()[:3] == [94, 95, 0]
    err = max_rel_err(text_embed_f64(sd, ids, 2), ref)
    print(f'fp64 restatement against the golden embeddings: {err:.3e}')
    assert err <= 1e-12


# ---- loader ---------------------------------------------------------------------------------------------------------------
def test_both_layouts_give_the_same_parameters_and_outputs():
    from rick_amd.cliptext import params_from_state_dict
    ids = text_prompts(3, 16, 96, seed=3)
    want_p = params_from_state_dict(synthetic_text_state_dict(CFG, 11))
    want = load(synthetic_text_state_dict(CFG, 11), heads=HEADS)(ids)
    sd = synthetic_text_state_dict(CFG, 11, 'openai')
    p = params_from_state_dict(sd)
    assert p.keys() == want_p.keys() and all(torch.equal(p[k], want_p[k]) for k in p)
    assert all(v.dtype == torch.float32 and v.is_contiguous() for v in p.values())
    assert torch.equal(load(sd, heads=HEADS)(ids), want)
    half = params_from_state_dict({k: v.half() for k, v in sd.items()})       # OpenAI checkpoints are fp16
    assert all(v.dtype == torch.float32 for v in half.values()) and torch.equal(half['tok'], want_p['tok'].half().float())


@pytest.mark.parametrize('layouts', [('transformers', 'transformers'), ('openai', 'openai-visual')])
def test_a_whole_model_checkpoint_loads_into_both_towers(layouts):
    from rick_amd.clip import ClipImageFeatures
    text_sd, image_sd = synthetic_text_state_dict(CFG, 11, layouts[0]), synthetic_clip_state_dict(IMAGE_CFG, 11, layouts[1])
    extra = {'logit_scale': torch.tensor(4.6)}
    if layouts[0] == 'transformers':
        extra.update({'text_model.embeddings.position_ids': torch.arange(16)[None], 'vision_model.embeddings.position_ids': torch.arange(17)[None]})
    else:
        extra.update({'input_resolution': torch.tensor(32), 'context_length': torch.tensor(16), 'vocab_size': torch.tensor(96)})
    both = {**text_sd, **image_sd, **extra}
    tnet, inet = load(both, heads=HEADS), ClipImageFeatures.load(both, device='cpu', heads=4)
    want_t, want_i = load(text_sd, heads=HEADS).params, ClipImageFeatures.load(image_sd, device='cpu', heads=4).params
    assert tnet.params.keys() == want_t.keys() and all(torch.equal(tnet.params[k], want_t[k]) for k in want_t)
    assert all(torch.equal(inet.params[k], want_i[k]) for k in want_i)
    assert tnet.cfg.dim == inet.cfg.dim == 32


@pytest.mark.parametrize('layout', ['transformers', 'openai'])
def test_unknown_and_missing_keys_raise(layout):
    sd = synthetic_text_state_dict(CFG, 11, layout)
    unknown = ('text_model.' if layout == 'transformers' else '') + 'surprise.weight'
    with pytest.raises(RuntimeError, match='surprise'):
        load({**sd, unknown: torch.zeros(3)}, heads=HEADS)
    for key in list(sd)[::5]:
        with pytest.raises(RuntimeError, match='missing key'):
            load({k: v for k, v in sd.items() if k != key}, heads=HEADS)
    with pytest.raises(RuntimeError, match='shape'):
        load({**sd, list(sd)[-2]: torch.zeros(3)}, heads=HEADS)


def test_the_configuration_is_read_from_the_shapes():
    c = load(synthetic_text_state_dict(CFG, 11, 'openai'), heads=HEADS).cfg
    assert (c.width, c.tokens, c.vocab, c.layers, c.mlp, c.dim, c.heads) == (64, 16, 96, 2, 256, 32, 4)
    assert load(synthetic_text_state_dict(CFG, 11)).cfg.heads == 1            # CLIP's rule: width / 64
    sd, _, _ = golden()
    g = load(sd, heads=2).cfg
    assert (g.width, g.tokens, g.vocab, g.layers, g.mlp, g.dim, g.heads) == (32, 12, 96, 2, 128, 16, 2)


def test_unsupported_configurations_are_refused_at_load():
    sd = synthetic_text_state_dict(CFG, 11)
    for heads in (8, 3, 0):                                                   # head dim 8; no divisor; nonsense
        with pytest.raises(RuntimeError, match='head'):
            load(sd, heads=heads)
    with pytest.raises(RuntimeError, match='multiple of 64'):
        load(synthetic_text_state_dict({**CFG, 'width': 32}, 11))            # no heads= and width / 64 is no integer
    with pytest.raises(RuntimeError, match='258 positions'):
        load(synthetic_text_state_dict({**CFG, 'tokens': 258}, 11), heads=HEADS)
    assert load(synthetic_text_state_dict({**CFG, 'tokens': 257, 'layers': 1}, 11), heads=HEADS).cfg.tokens == 257
    with pytest.raises(RuntimeError, match='width 66'):
        load(synthetic_text_state_dict({**CFG, 'width': 66}, 11), heads=HEADS)
    with pytest.raises(RuntimeError, match='MLP width 254'):
        load(synthetic_text_state_dict({**CFG, 'mlp': 254}, 11), heads=HEADS)
    with pytest.raises(RuntimeError, match='width 2112'):
        load(synthetic_text_state_dict({**CFG, 'width': 2112, 'layers': 1, 'mlp': 4, 'vocab': 4}, 11))
    with pytest.raises(ValueError, match='batch'):
        load(sd, heads=HEADS, batch=0)
    pos = 'text_model.embeddings.position_embedding.weight'
    for bad in (torch.zeros(16), torch.zeros(16, 32), torch.zeros(1, 16, 64)):
        with pytest.raises(RuntimeError, match=r'position_embedding.*expected \(T, 64\)'):
            load({**sd, pos: bad}, heads=HEADS)


def test_bad_ids_are_refused():
    net = load(synthetic_text_state_dict(CFG, 11), heads=HEADS)
    ids = text_prompts(2, 16, 96, seed=1)
    for bad in (96, -1, 1 << 40):
        with pytest.raises(ValueError, match='outside the vocabulary'):
            net(torch.where(ids == 95, torch.tensor(bad), ids))
    with pytest.raises(ValueError, match='15 positions'):
        net(ids[:, :15])
    with pytest.raises(ValueError, match='17 positions'):
        net(torch.cat([ids, ids[:, :1]], 1))
    with pytest.raises(RuntimeError, match='integer'):
        net(ids.float())
    with pytest.raises(RuntimeError, match='expected ids'):
        net(ids[0])
    assert tuple(net(ids[:0]).shape) == (0, 32)
    assert torch.equal(net(ids.to(torch.int32)), net(ids))


def test_row_numbers_out_of_range_are_refused_on_the_host():
    from rick_amd.cliptext import check_rows
    assert check_rows(torch.tensor([4, 0, 4, 2]), 5).tolist() == [4, 0, 4, 2] and check_rows(torch.tensor([1]), 5).dtype == torch.int32
    for bad in ([0, 5], [-1], [1 << 33]):
        with pytest.raises(ValueError, match='outside the 5 rows'):
            check_rows(torch.tensor(bad), 5)
    with pytest.raises(RuntimeError, match='integer'):
        check_rows(torch.tensor([1.0]), 5)


# ---- the fp32 composition -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', list(NET_CPU_BASE))
def test_cpu_path_vs_fp64(n):
    sd = synthetic_text_state_dict(CFG, 11)
    ids = text_prompts(n, 16, 96, seed=n)
    got = load(sd, heads=HEADS, batch=4)(ids)                                 # n = 9: chunks of 4 + 4 + 1
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, 32)
    err, base = max_rel_err(got, text_embed_f64(sd, ids, HEADS)), NET_CPU_BASE[n]
    print(f'CLIP text on the CPU, n={n}: max err / max-norm {err:.3e} (measured {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base


def test_cpu_path_on_the_golden():
    sd, ids, ref = golden()
    err = max_rel_err(load(sd, heads=2)(ids), ref)
    print(f'CLIP text on the CPU, golden: {err:.3e} (measured {GOLDEN_CPU_BASE:.3e}, bound {FACTOR * GOLDEN_CPU_BASE:.3e})')
    assert err <= FACTOR * GOLDEN_CPU_BASE


def test_ids_behind_the_first_eot_do_not_matter():
    sd = synthetic_text_state_dict(CFG, 11)
    net = load(sd, heads=HEADS)
    ids = text_prompts(3, 16, 96, seed=3)
    want = net(ids)
    ref = text_embed_f64(sd, ids, HEADS)
    gen = torch.Generator().manual_seed(4)
    for pad in (95, 7, 'random'):
        other = ids.clone()
        for r in range(3):
            e = first_max(ids[r].tolist())
            other[r, e + 1:] = torch.randint(0, 96, (15 - e,), generator=gen) if pad == 'random' else pad      # 95 again: still the first
        assert torch.equal(text_embed_f64(sd, other, HEADS), ref)              # the restatement does not see them at all
        err = max_rel_err(net(other), ref)
        print(f'ids behind EOT = {pad}: {err:.3e} (bound {FACTOR * NET_CPU_BASE[3]:.3e})')
        assert err <= FACTOR * NET_CPU_BASE[3]
        assert max_rel_err(net(other), want.double()) <= FACTOR * NET_CPU_BASE[3]


def test_the_eot_row_is_the_first_maximum():
    from rick_amd.cliptext import eot_positions
    ids = torch.tensor([[94, 3, 95, 95, 0], [94, 95, 0, 0, 0], [5, 5, 5, 5, 5], [1, 2, 3, 4, 9], [94, 7, 60, 2, 1]])
    assert eot_positions(ids).tolist() == [2, 1, 0, 4, 0]
    assert eot_positions(ids).tolist() == [first_max(r) for r in ids.tolist()]
    sd = synthetic_text_state_dict(CFG, 11)
    net = load(sd, heads=HEADS)
    row = text_prompts(3, 16, 96, seed=3)[2:3].clone()
    e = first_max(row[0].tolist())
    assert 1 < e < 15
    late = row.clone()
    late[0, e], late[0, e + 1] = 3, 95                                        # EOT one position later: another row is pooled
    assert max_rel_err(net(late), net(row).double()) > 1e-3


# ---- tokenizer ------------------------------------------------------------------------------------------------------------
def test_tokenizer_reproduces_every_golden_id_row():
    tok, z = golden_tokenizer()
    texts, want = json.loads(str(z['tok_texts'])), torch.from_numpy(z['tok_ids'])
    assert want.dtype == torch.int64 and tuple(want.shape) == (len(texts), tok.context) and tok.eot_id == max(tok.vocab.values())
    tok_pad = golden_tokenizer(pad_id=int(z['tok_pad_id']))[0]
    for i, text in enumerate(texts):
        got = tok_pad([text], truncate=True)
        assert got.dtype == torch.int64 and torch.equal(got[0], want[i]), (text, got[0].tolist(), want[i].tolist())
    assert torch.equal(tok_pad(texts, truncate=True), want)
    mine = tok(texts, truncate=True)                                          # pad_id 0: the same row up to its closing EOT, then 0
    for i in range(len(texts)):
        row = want[i].tolist()
        end = max(k for k in range(len(row)) if row[k] != tok.eot_id) + 1     # the library pads with EOT: the first of the final run
        assert mine[i].tolist() == row[:end + 1] + [0] * (len(row) - end - 1)
    assert torch.equal(tok('the dog'), tok(['the dog']))


def test_tokenizer_steps():
    from rick_amd.cliptok import byte_table, normalise, pre_tokens
    table = byte_table()
    assert len(set(table.values())) == 256 and table[ord('a')] == 'a' and table[ord(' ')] == 'Ġ' and table[0] == 'Ā'
    assert normalise('  Café \t\n X ') == ' café x '
    assert pre_tokens("he'd 12ab!!'s <|endoftext|>x") == ['he', "'d", '1', '2', 'ab', "!!'", 's', '<|', 'endoftext', '|>', 'x']
    tok, _ = golden_tokenizer()
    assert tok.encode('dog!<|endoftext|>The') == tok.encode('dog!') + [tok.eot_id] + tok.encode('the')      # cut out of the raw text
    assert tok.eot_id not in tok.encode('a <|ENDOFTEXT|> b') and tok.encode('<|ENDOFTEXT|>') == tok.encode('<| endoftext |>')
    assert tok.bpe('the') == ['the</w>'] and tok.bpe('photo') == ['photo</w>'] and tok.bpe('then') == ['th', 'e', 'n</w>']


def test_over_long_input_raises_without_truncate():
    tok, z = golden_tokenizer()
    texts = json.loads(str(z['tok_texts']))
    long = [int(i) for i in z['tok_long']]
    assert long
    for i, text in enumerate(texts):
        if i in long:
            with pytest.raises(ValueError, match='context is 48'):
                tok([text])
            row = tok([text], truncate=True)[0]
            assert row[0] == tok.bos_id and row[-1] == tok.eot_id and first_max(row.tolist()) == tok.context - 1
        else:
            assert tuple(tok([text]).shape) == (1, 48)
    with pytest.raises(ValueError, match='startoftext'):
        from rick_amd.cliptok import ClipTokenizer
        ClipTokenizer({'<|endoftext|>': 0}, [])


def test_tokenizer_loads_its_files(tmp_path):
    from rick_amd.cliptok import ClipTokenizer
    tok, z = golden_tokenizer()
    (tmp_path / 'vocab.json').write_text(str(z['tok_vocab']), encoding='utf-8')
    (tmp_path / 'merges.txt').write_text('#version: 0.2\n' + str(z['tok_merges']) + '\n', encoding='utf-8')
    loaded = ClipTokenizer.load(str(tmp_path / 'vocab.json'), str(tmp_path / 'merges.txt'), context=48)
    texts = json.loads(str(z['tok_texts']))
    assert torch.equal(loaded(texts, truncate=True), tok(texts, truncate=True))


# ---- the text direction ---------------------------------------------------------------------------------------------------
def test_text_direction_is_the_formula_and_clipguide_accepts_it():
    from rick_amd.clip import ClipImageFeatures
    from rick_amd.clipguide import ClipGuide, directional_loss, text_direction
    tok, _ = golden_tokenizer()
    sd = synthetic_text_state_dict(TOK_CFG, 5)
    tnet = load(sd, heads=TOK_HEADS)
    got = text_direction(tnet, tok, 'dog', 'photo', TEMPLATES)
    assert got.dtype == torch.float32 and tuple(got.shape) == (16,) and abs(float(got.double().norm()) - 1) < 1e-6
    e_s, e_t = (text_embed_f64(sd, tok([t.format(w) for t in TEMPLATES]), TOK_HEADS) for w in ('dog', 'photo'))
    err = max_rel_err(got, direction_f64(e_s, e_t))
    print(f'text_direction on the CPU: {err:.3e} (measured {DIRECTION_CPU_BASE:.3e}, bound {FACTOR * DIRECTION_CPU_BASE:.3e})')
    assert err <= FACTOR * DIRECTION_CPU_BASE
    one = text_direction(tnet, tok, 'dog', 'photo')                           # the default template
    assert max_rel_err(one, direction_f64(*(text_embed_f64(sd, tok([f'a photo of a {w}.']), TOK_HEADS) for w in ('dog', 'photo')))) \
        <= FACTOR * DIRECTION_CPU_BASE
    with pytest.raises(ValueError, match='coincide'):
        text_direction(tnet, tok, 'dog', 'dog')
    inet = ClipImageFeatures.load(synthetic_clip_state_dict({**IMAGE_CFG, 'dim': 16}, 11), device='cpu', heads=4)
    guide = ClipGuide(inet, got)
    assert torch.equal(guide.direction, got)
    e = torch.randn(4, 16, generator=torch.Generator().manual_seed(2))
    assert torch.isfinite(directional_loss(e, e.flip(0), got))
