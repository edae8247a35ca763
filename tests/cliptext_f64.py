"""Independent fp64 restatement of CLIP's text tower, written from the specification (one prompt and one query row at a
time, explicit loops over the visible keys, no mask tensor, no torch.nn.functional network ops):

1. t[i] = token_embedding[ids[i]] + positional_embedding[i];
2. L blocks: t += out_proj(attention(ln_1 t)); t += c_proj(quickgelu(c_fc(ln_2 t))), quickgelu(u) = u / (1 + exp(-1.702 u));
   head h owns columns [h d, (h + 1) d); query row i is the softmax over the keys 0 .. i ONLY of q_i . k_j / sqrt(d), times v;
3. ln_final (eps 1e-5, biased variance) on the row of the first occurrence of the row's largest id;
4. the projection without bias.

It reads a state_dict in the transformers layout.  Plus synthetic weights in both layouts, seeded prompts, the direction
formula and the error measure.  Nothing here imports rick_amd.cliptext."""
import math

import torch

from tests.vgg_f64 import max_rel_err  # noqa: F401  (re-exported)


def _ln(x, w, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * w + b


def first_max(row):
    """The first position of the largest id of a row (a list of ints)."""
    return row.index(max(row))


def text_embed_f64(sd, ids, heads):
    """ids [N, T] integer -> text embeddings [N, D] fp64; sd in the transformers layout."""
    g = lambda k: sd[k].double()                                              # noqa: E731
    table, pos = g('text_model.embeddings.token_embedding.weight'), g('text_model.embeddings.position_embedding.weight')
    T, wd = pos.shape
    assert ids.shape[1] == T
    layers = 1 + max(int(k.split('.')[3]) for k in sd if k.startswith('text_model.encoder.layers.'))
    d = wd // heads
    out = []
    for row in ids.tolist():
        t = torch.stack([table[row[i]] + pos[i] for i in range(T)])
        for layer in range(layers):
            pre = f'text_model.encoder.layers.{layer}.'
            lin = lambda v, name: v @ g(pre + name + '.weight').T + g(pre + name + '.bias')      # noqa: E731
            h = _ln(t, g(pre + 'layer_norm1.weight'), g(pre + 'layer_norm1.bias'))
            q, k, v = (lin(h, f'self_attn.{n}_proj') for n in 'qkv')
            att = torch.zeros_like(q)
            for hd in range(heads):
                c = slice(hd * d, (hd + 1) * d)
                for i in range(T):                            # the keys 0 .. i and no others
                    s = k[:i + 1, c] @ q[i, c] / math.sqrt(d)
                    e = torch.exp(s - s.max())
                    att[i, c] = (e / e.sum()) @ v[:i + 1, c]
            t = t + lin(att, 'self_attn.out_proj')
            u = lin(_ln(t, g(pre + 'layer_norm2.weight'), g(pre + 'layer_norm2.bias')), 'mlp.fc1')
            t = t + lin(u / (1 + torch.exp(-1.702 * u)), 'mlp.fc2')
        eot = _ln(t[first_max(row)], g('text_model.final_layer_norm.weight'), g('text_model.final_layer_norm.bias'))
        out.append(eot @ g('text_projection.weight').T)
    return torch.stack(out)


def direction_f64(e_source, e_target):
    """n(mean_t n(e_target,t) - mean_t n(e_source,t)) in fp64 from [templates, D] embeddings."""
    n = lambda e: e / e.norm(dim=-1, keepdim=True)                            # noqa: E731
    return n(n(e_target.double()).mean(0) - n(e_source.double()).mean(0))


# ---- synthetic weights ----------------------------------------------------------------------------------------------------
def synthetic_text_state_dict(cfg, seed, layout='transformers'):
    """cfg: dict(width, tokens, vocab, layers, mlp, dim).  The same seeded fp32 weights in the 'transformers' or the 'openai'
    layout.  Fan-in-scaled normals keep the residual stream O(1); LayerNorm weights are spread around 1 and every bias is
    non-zero."""
    wd, T, V, L, M, D = cfg['width'], cfg['tokens'], cfg['vocab'], cfg['layers'], cfg['mlp'], cfg['dim']
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s, std=1.0: torch.randn(*s, generator=gen) * std            # noqa: E731
    lnw = lambda: 1 + 0.2 * rn(wd)                                            # noqa: E731
    hf = layout == 'transformers'
    sd = {}
    table, pos = rn(V, wd, std=0.5), rn(T, wd, std=0.3)
    if hf:
        sd['text_model.embeddings.token_embedding.weight'], sd['text_model.embeddings.position_embedding.weight'] = table, pos
    else:
        sd['token_embedding.weight'], sd['positional_embedding'] = table, pos
    for i in range(L):
        qkv_w, qkv_b = rn(3 * wd, wd, std=wd ** -0.5), rn(3 * wd, std=0.1)
        ln1, ln2 = (lnw(), rn(wd, std=0.1)), (lnw(), rn(wd, std=0.1))
        out, fc, proj = (rn(wd, wd, std=wd ** -0.5), rn(wd, std=0.05)), (rn(M, wd, std=wd ** -0.5), rn(M, std=0.1)), \
            (rn(wd, M, std=M ** -0.5), rn(wd, std=0.05))
        if hf:
            b = f'text_model.encoder.layers.{i}.'
            for j, n in enumerate('qkv'):
                sd[f'{b}self_attn.{n}_proj.weight'] = qkv_w[j * wd:(j + 1) * wd].clone()
                sd[f'{b}self_attn.{n}_proj.bias'] = qkv_b[j * wd:(j + 1) * wd].clone()
            named = (('layer_norm1', ln1), ('self_attn.out_proj', out), ('layer_norm2', ln2), ('mlp.fc1', fc), ('mlp.fc2', proj))
        else:
            b = f'transformer.resblocks.{i}.'
            sd[b + 'attn.in_proj_weight'], sd[b + 'attn.in_proj_bias'] = qkv_w, qkv_b
            named = (('ln_1', ln1), ('attn.out_proj', out), ('ln_2', ln2), ('mlp.c_fc', fc), ('mlp.c_proj', proj))
        for name, (w, bias) in named:
            sd[f'{b}{name}.weight'], sd[f'{b}{name}.bias'] = w, bias
    ln = 'text_model.final_layer_norm' if hf else 'ln_final'
    sd[ln + '.weight'], sd[ln + '.bias'] = lnw(), rn(wd, std=0.1)
    head = rn(D, wd, std=wd ** -0.5)
    if hf:
        sd['text_projection.weight'] = head
    else:
        sd['text_projection'] = head.t().contiguous()
    return sd


def text_prompts(n, tokens, vocab, seed, pad=0):
    """n id rows [n, tokens] int64: BOS = vocab - 2, a seeded number (0 .. tokens - 2) of ids below BOS, EOT = vocab - 1, then
    `pad`.  Row 0 is BOS, EOT alone and row 1 fills every position."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((n, tokens), pad, dtype=torch.int64)
    for i in range(n):
        m = 0 if i == 0 else tokens - 2 if i == 1 else int(torch.randint(0, tokens - 1, (1,), generator=g))
        ids[i, 0] = vocab - 2
        ids[i, 1:1 + m] = torch.randint(0, vocab - 2, (m,), generator=g)
        ids[i, 1 + m] = vocab - 1
    return ids
