"""GPU: the CLIP text-tower kernels (rick_clip_text_tokens_f32, rick_clip_attention_causal_f32, rick_clip_layernorm_rows_f32 in
rick_amd/csrc/clip.hip) through the C ABI, bit for bit against what they restate (the fp32 sum formed on the CPU, the unmasked
attention kernel on every prefix, the LayerNorm kernel on gathered rows) and against fp64; the whole network
(rick_amd/cliptext.py) against the independent fp64 restatement (tests/cliptext_f64.py) and against the golden embeddings of
an implementation the author did not write; batch and padding invariance; the text direction.  The conftest's autouse
fixture asserts after every test that the saturation counter stayed at 0.

Tolerances: the rule of tests/test_gpu_vgg.py and tests/test_gpu_clip.py.  For every comparison the base figure is the error of
the fp32 torch CPU composition against the same fp64 reference on the same inputs (max error over the reference's max-norm,
measured once on the CPU and written down below next to its shape); the device bound is that figure x 4."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.cliptext_f64 import direction_f64, first_max, max_rel_err, synthetic_text_state_dict, text_embed_f64, text_prompts

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENTINEL = 12345.0
FACTOR = 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'clip_text_tiny.npz')

# fp32 torch CPU softmax(q k^T / sqrt(d) + mask) v against the fp64 masked softmax on attention_inputs(T, d, heads)
ATT_SHAPES = [(13, 16, 2), (77, 64, 2), (130, 32, 1)]                         # (T, d, heads); 130 crosses the 64- and 128-key slots
ATT_CPU_BASE = {(13, 16, 2): 1.434e-07, (77, 64, 2): 3.310e-07, (130, 32, 1): 1.165e-07}
# fp32 torch CPU network (ClipTextFeatures on CPU ids) against the fp64 restatement on network_inputs(name)[:n]
NET_CPU_BASE = {('A', 3): 3.670e-07, ('A', 70): 5.161e-07, ('B', 3): 3.373e-07, ('B', 70): 4.278e-07}
GOLDEN_CPU_BASE = 4.510e-07                                      # the golden's weights and ids against the golden's embeddings
# text_direction with the fp32 torch CPU network against direction_f64 of the restatement's embeddings: network C, 'dog' ->
# 'photo', TEMPLATES
DIRECTION_CPU_BASE = 5.288e-07
TEMPLATES = ('a photo of a {}.', 'the {}!', '{}')

CONFIGS = {'A': (dict(width=64, tokens=16, vocab=96, layers=2, mlp=256, dim=32), 4),        # (cfg, heads): d = 16
           'B': (dict(width=128, tokens=77, vocab=512, layers=1, mlp=512, dim=64), 2),      # d = 64
           'C': (dict(width=64, tokens=48, vocab=529, layers=1, mlp=128, dim=32), 4)}       # the golden tokenizer's context and vocabulary


def _lib():
    from rick_amd import _lib
    return _lib


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- token embedding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,T,V,C', [(3, 12, 96, 32), (2, 77, 512, 132)])
def test_tokens_kernel_is_the_fp32_sum(N, T, V, C):
    L = _lib()
    g = _gen(N * 1000 + C)
    ids = torch.randint(0, V, (N, T), generator=g, dtype=torch.int32)
    ids[0, 0], ids[0, 1], ids[-1, -1], ids[-1, -2] = 0, V - 1, V - 1, 0
    table, pos = torch.randn(V, C, generator=g), torch.randn(T, C, generator=g)
    out = torch.full((N * T + 1, C), SENTINEL, device=DEV)                      # one guard row behind the output
    dev = [v.to(DEV) for v in (ids, table, pos)]
    L.check(L.lib.rick_clip_text_tokens_f32(*(v.data_ptr() for v in dev), out.data_ptr(), N, T, V, C, L.stream_ptr()),
            'rick_clip_text_tokens_f32')
    assert torch.all(out[N * T] == SENTINEL)
    assert torch.equal(out[:N * T].cpu().view(N, T, C), table[ids.long()] + pos)


def test_tokens_kernel_rejects_what_it_does_not_support():
    L = _lib()
    t = torch.zeros(1 << 14, device=DEV)
    i = torch.zeros(64, device=DEV, dtype=torch.int32)
    p, q, s = t.data_ptr(), i.data_ptr(), L.stream_ptr()
    assert L.lib.rick_clip_text_tokens_f32(q, p, p, p, 2, 5, 7, 16, s) == 0
    for N, T, V, C in ((2, 5, 7, 18), (2, 258, 7, 16), (2, 0, 7, 16), (2, 5, 0, 16), (-1, 5, 7, 16), (2, 5, 7, 2052),
                       ((1 << 31) // 257, 257, 7, 2048)):                  # N T fits an int, the grid does not
        assert L.lib.rick_clip_text_tokens_f32(q, p, p, p, N, T, V, C, s) == 22
    assert L.lib.rick_clip_text_tokens_f32(None, p, p, p, 2, 5, 7, 16, s) == 22
    torch.cuda.synchronize()


# ---- causal attention -----------------------------------------------------------------------------------------------------
def attention_inputs(T, d, heads):
    return torch.randn(3, T, 3 * heads * d, generator=_gen(T * 100 + d))


def causal_reference_f64(qkv, d, heads):
    """Row i: the softmax over the keys 0 .. i only, in fp64, one row at a time."""
    n, T, _ = qkv.shape
    wd = heads * d
    x = qkv.double()
    out = torch.zeros(n, T, wd, dtype=torch.float64)
    for b in range(n):
        for h in range(heads):
            q, k, v = (x[b, :, j * wd + h * d:j * wd + (h + 1) * d] for j in range(3))
            for i in range(T):
                s = k[:i + 1] @ q[i] / math.sqrt(d)
                e = torch.exp(s - s.max())
                out[b, i, h * d:(h + 1) * d] = (e / e.sum()) @ v[:i + 1]
    return out


def run_attention(qkv, d, heads, causal=True):
    L = _lib()
    n, T, _ = qkv.shape
    qd = qkv.to(DEV).contiguous()
    out = torch.full((n * T + 1, heads * d), SENTINEL, device=DEV)
    fn = L.lib.rick_clip_attention_causal_f32 if causal else L.lib.rick_clip_attention_f32
    L.check(fn(qd.data_ptr(), out.data_ptr(), n, T, heads, d, L.stream_ptr()), 'rick_clip_attention')
    assert torch.all(out[n * T] == SENTINEL)
    return out[:n * T].view(n, T, heads * d).cpu()


_ATT = {}


def causal_output(T, d, heads):
    if (T, d, heads) not in _ATT:
        _ATT[(T, d, heads)] = run_attention(attention_inputs(T, d, heads), d, heads)
    return _ATT[(T, d, heads)]


@pytest.mark.parametrize('T,d,heads', ATT_SHAPES)
def test_causal_row_is_the_unmasked_kernel_on_its_prefix(T, d, heads):
    qkv, got = attention_inputs(T, d, heads), causal_output(T, d, heads)
    rows = sorted({i for i in (0, 1, 62, 63, 64, 65, 127, 128, T - 2, T - 1) if 0 <= i < T})
    assert rows
    for i in rows:
        prefix = run_attention(qkv[:, :i + 1].contiguous(), d, heads, causal=False)
        assert torch.equal(got[:, i], prefix[:, i]), f'row {i}'


@pytest.mark.parametrize('T,d,heads', ATT_SHAPES)
def test_causal_rows_do_not_see_later_rows(T, d, heads):
    qkv, got = attention_inputs(T, d, heads), causal_output(T, d, heads)
    for i in sorted({i for i in (0, 63, 64, T - 2) if 0 <= i < T - 1}):
        other = qkv.clone()
        other[:, i + 1:] = torch.randn(3, T - i - 1, qkv.shape[2], generator=_gen(i)) * 5
        assert torch.equal(run_attention(other, d, heads)[:, :i + 1], got[:, :i + 1]), f'rows <= {i}'


@pytest.mark.parametrize('T,d,heads', ATT_SHAPES)
def test_causal_attention_vs_fp64(T, d, heads):
    qkv, got = attention_inputs(T, d, heads), causal_output(T, d, heads)
    err, base = max_rel_err(got, causal_reference_f64(qkv, d, heads)), ATT_CPU_BASE[(T, d, heads)]
    print(f'rick_clip_attention_causal_f32 T={T} d={d} heads={heads}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, '
          f'bound {FACTOR * base:.3e})')
    assert torch.isfinite(got).all()
    assert err <= FACTOR * base
    assert torch.equal(run_attention(qkv, d, heads), got)                     # run to run


@pytest.mark.parametrize('T,d,heads', ATT_SHAPES)
def test_causal_attention_of_a_prompt_does_not_depend_on_the_batch(T, d, heads):
    qkv, full = attention_inputs(T, d, heads), causal_output(T, d, heads)
    assert torch.equal(run_attention(qkv[1:2], d, heads), full[1:2])          # alone
    assert torch.equal(run_attention(qkv.flip(0), d, heads)[2], full[0])      # last in a flipped batch
    other = torch.randn(qkv.shape, generator=_gen(9))
    other[1] = qkv[1]
    assert torch.equal(run_attention(other, d, heads)[1], full[1])            # beside different prompts


def test_causal_attention_rejects_what_it_does_not_support():
    L = _lib()
    t = torch.zeros(1 << 16, device=DEV)
    p, s = t.data_ptr(), L.stream_ptr()
    assert L.lib.rick_clip_attention_causal_f32(p, p, 1, 5, 2, 16, s) == 0
    for T, heads, d in ((258, 1, 16), (0, 1, 16), (5, 2, 48), (5, 2, 128), (5, 0, 16)):
        assert L.lib.rick_clip_attention_causal_f32(p, p, 1, T, heads, d, s) == 22
    assert L.lib.rick_clip_attention_causal_f32(None, p, 1, 5, 2, 16, s) == 22
    torch.cuda.synchronize()


# ---- LayerNorm of rows picked by index ------------------------------------------------------------------------------------
def layernorm_inputs(R, C):
    g = _gen(R * 10000 + C)
    return torch.randn(R, C, generator=g) * 1.5 + 0.3, 1 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)


@pytest.mark.parametrize('R,C,idx', [(51, 64, [50, 0, 17, 17, 3, 49, 0, 33, 16]), (9, 768, [8, 8, 0, 5, 1, 0, 7])])
def test_layernorm_rows_is_the_layernorm_kernel_on_the_gathered_rows(R, C, idx):
    from rick_amd.cliptext import layernorm_rows
    L = _lib()
    x, w, b = (v.to(DEV) for v in layernorm_inputs(R, C))
    n = len(idx)
    gathered = x[torch.tensor(idx, device=DEV)].contiguous()
    want = torch.empty(n, C, device=DEV)
    L.check(L.lib.rick_clip_layernorm_f32(gathered.data_ptr(), C, w.data_ptr(), b.data_ptr(), want.data_ptr(), n, C, 1e-5, L.stream_ptr()),
            'rick_clip_layernorm_f32')
    out = torch.full((n + 1, C), SENTINEL, device=DEV)
    di = torch.tensor(idx, dtype=torch.int32, device=DEV)
    L.check(L.lib.rick_clip_layernorm_rows_f32(x.data_ptr(), di.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), n, C, 1e-5,
                                               L.stream_ptr()), 'rick_clip_layernorm_rows_f32')
    assert torch.all(out[n] == SENTINEL)
    assert torch.equal(out[:n], want)
    assert torch.equal(layernorm_rows(x, torch.tensor(idx), w, b), want)      # the host wrapper: the same launch


def test_layernorm_rows_refuses_an_index_out_of_range_on_the_host():
    from rick_amd.cliptext import layernorm_rows
    L = _lib()
    x, w, b = (v.to(DEV) for v in layernorm_inputs(51, 64))
    for bad in ([0, 51], [-1, 3], [1 << 31]):
        with pytest.raises(ValueError, match='outside the 51 rows'):
            layernorm_rows(x, torch.tensor(bad), w, b)
    t, rows = torch.zeros(1 << 14, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    p, i, s = t.data_ptr(), rows.data_ptr(), L.stream_ptr()
    assert L.lib.rick_clip_layernorm_rows_f32(p, i, p, p, p, 4, 64, 1e-5, s) == 0
    for R, C in ((4, 62), (4, 2052), (-1, 64)):
        assert L.lib.rick_clip_layernorm_rows_f32(p, i, p, p, p, R, C, 1e-5, s) == 22
    assert L.lib.rick_clip_layernorm_rows_f32(p, None, p, p, p, 4, 64, 1e-5, s) == 22
    torch.cuda.synchronize()


# ---- whole network --------------------------------------------------------------------------------------------------------
_NETS, _NET_REF = {}, {}


def network(name, layout='transformers'):
    from rick_amd.cliptext import ClipTextFeatures
    if (name, layout) not in _NETS:
        cfg, heads = CONFIGS[name]
        _NETS[(name, layout)] = ClipTextFeatures.load(synthetic_text_state_dict(cfg, 11, layout), device=DEV, heads=heads)
    return _NETS[(name, layout)]


def network_inputs(name):
    cfg, _ = CONFIGS[name]
    return text_prompts(70, cfg['tokens'], cfg['vocab'], seed=ord(name))


def network_reference(name):
    if name not in _NET_REF:
        cfg, heads = CONFIGS[name]
        _NET_REF[name] = text_embed_f64(synthetic_text_state_dict(cfg, 11), network_inputs(name), heads)
    return _NET_REF[name]


@pytest.mark.parametrize('name,n', list(NET_CPU_BASE))
def test_network_vs_fp64(name, n):
    net = network(name)
    assert net.batch == 64                                    # 70 prompts: chunks of 64 + 6
    ids = network_inputs(name)[:n].to(DEV)
    got = net(ids)
    assert got.dtype == torch.float32 and tuple(got.shape) == (n, CONFIGS[name][0]['dim']) and got.device.type == 'cuda'
    err, base = max_rel_err(got.cpu(), network_reference(name)[:n]), NET_CPU_BASE[(name, n)]
    print(f'CLIP text {name}, n={n}: max err / max-norm {err:.3e} (fp32 CPU {base:.3e}, bound {FACTOR * base:.3e})')
    assert err <= FACTOR * base
    assert torch.equal(net(ids), got)                                         # run to run


def test_network_on_the_golden_weights_vs_the_golden_embeddings():
    from rick_amd.cliptext import ClipTextFeatures
    z = np.load(GOLDEN)
    sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith('sd/')}
    net = ClipTextFeatures.load(sd, device=DEV, heads=2)
    got = net(torch.from_numpy(z['ids']).to(DEV))
    err = max_rel_err(got.cpu(), torch.from_numpy(z['text_embeds']))
    print(f'CLIP text golden: max err / max-norm {err:.3e} (fp32 CPU {GOLDEN_CPU_BASE:.3e}, bound {FACTOR * GOLDEN_CPU_BASE:.3e})')
    assert err <= FACTOR * GOLDEN_CPU_BASE


@pytest.mark.parametrize('name', ['A', 'B'])
def test_both_layouts_give_the_same_bits(name):
    ids = network_inputs(name)[:5].to(DEV)
    assert torch.equal(network(name, 'openai')(ids), network(name)(ids))


@pytest.mark.parametrize('name', ['A', 'B'])
def test_embeddings_do_not_depend_on_the_batch_or_on_the_ids_behind_eot(name):
    net = network(name)
    cpu = network_inputs(name)
    ids = cpu.to(DEV)
    full = net(ids)                                           # chunks of 64 + 6
    assert torch.equal(net(ids[:3]), full[:3])
    assert torch.equal(net(ids[63:66]), full[63:66])          # prompt 63: last of a chunk there, first of one here
    assert torch.equal(net(ids[69:70]), full[69:70])
    assert torch.equal(net(ids.flip(0)).flip(0), full)
    assert torch.equal(net(cpu.to(torch.int32).to(DEV)), full)
    vocab, gen = CONFIGS[name][0]['vocab'], _gen(12)
    for pad in (vocab - 1, 7, 'random'):
        other = cpu.clone()
        for r in range(cpu.shape[0]):
            e = first_max(cpu[r].tolist())
            n = cpu.shape[1] - e - 1
            other[r, e + 1:] = torch.randint(0, vocab, (n,), generator=gen) if pad == 'random' else pad
        assert not torch.equal(other, cpu)
        assert torch.equal(net(other.to(DEV)), full), f'ids behind EOT = {pad}'


def test_ids_out_of_range_are_refused_before_upload():
    net = network('A')
    ids = network_inputs('A')[:2].clone()
    ids[1, 3] = 96
    with pytest.raises(ValueError, match='outside the vocabulary'):
        net(ids.to(DEV))
    with pytest.raises(ValueError, match='15 positions'):
        net(network_inputs('A')[:2, :15].to(DEV))


def test_text_direction_on_the_device_vs_the_fp64_formula():
    from rick_amd.clip import ClipImageFeatures
    from rick_amd.clipguide import ClipGuide, text_direction
    from rick_amd.cliptok import ClipTokenizer
    from tests.clip_f64 import synthetic_clip_state_dict
    z = np.load(GOLDEN)
    tok = ClipTokenizer(json.loads(str(z['tok_vocab'])), [tuple(line.split(' ')) for line in str(z['tok_merges']).split('\n')],
                        context=int(z['tok_context']))
    cfg, heads = CONFIGS['C']
    sd = synthetic_text_state_dict(cfg, 11)
    got = text_direction(network('C'), tok, 'dog', 'photo', TEMPLATES)
    assert got.dtype == torch.float32 and tuple(got.shape) == (32,) and got.device.type == 'cuda'
    e_s, e_t = (text_embed_f64(sd, tok([t.format(w) for t in TEMPLATES]), heads) for w in ('dog', 'photo'))
    err = max_rel_err(got.cpu(), direction_f64(e_s, e_t))
    print(f'text_direction on the device: {err:.3e} (fp32 CPU {DIRECTION_CPU_BASE:.3e}, bound {FACTOR * DIRECTION_CPU_BASE:.3e})')
    assert err <= FACTOR * DIRECTION_CPU_BASE
    assert torch.equal(text_direction(network('C'), tok, 'dog', 'photo', TEMPLATES), got)
    inet = ClipImageFeatures.load(synthetic_clip_state_dict(dict(width=64, patch=8, image=32, layers=1, mlp=256, dim=32), 11), device=DEV,
                                  batch=2, heads=4)
    assert torch.equal(ClipGuide(inet, got).direction, got)
