"""fp64 expressions of the style path (rick_amd/csrc/modulation.hip) and of the short-batch linear family
(rick_amd/csrc/linear.hip), written out from the formulas of include/rick_hip.h for tests/test_gpu_mod_forms.py.  Every function
takes fp32 CPU tensors and fp32-representable Python floats and returns (ref, S): the result and sum |terms| per output
element, both fp64.  A plain module: no fixtures, no device."""
import torch


def wsq(w, scale):
    """wsq[o,i] = scale^2 sum_k w[o,i,k]^2 (every term is positive: S = ref)."""
    ref = scale * scale * (w.double() ** 2).sum(-1)
    return ref, ref.clone()


def demod_sum(s, wsq_):
    """tot[b,o] = sum_i s[b,i]^2 wsq[o,i]"""
    return torch.einsum('bi,oi->bo', s.double() ** 2, wsq_.double())


def demod(s, wsq_, eps):
    """d[b,o] = rsqrt(sum_i s[b,i]^2 wsq[o,i] + eps) -> (d, tot)"""
    tot = demod_sum(s, wsq_)
    return (tot + eps) ** -0.5, tot


def tcoef(d, gd):
    """t[b,o] = -0.5 d^3 gd"""
    return -0.5 * d.double() ** 3 * gd.double()


def demod_bwd_s(s, wsq_, d, gd):
    """gs[b,i] = 2 s[b,i] sum_o t[b,o] wsq[o,i]"""
    t = tcoef(d, gd)
    ref = 2 * s.double() * torch.einsum('bo,oi->bi', t, wsq_.double())
    S = 2 * s.double().abs() * torch.einsum('bo,oi->bi', t.abs(), wsq_.double().abs())
    return ref, S


def demod_bwd_w(w, s, d, gd, scale, old=None):
    """gw[o,i,k] (+)= 2 scale^2 w[o,i,k] sum_b t[b,o] s[b,i]^2"""
    t, s2 = tcoef(d, gd), s.double() ** 2
    f = 2 * scale * scale * torch.einsum('bo,bi->oi', t, s2)
    F = 2 * scale * scale * torch.einsum('bo,bi->oi', t.abs(), s2)
    ref, S = w.double() * f[:, :, None], w.double().abs() * F[:, :, None]
    if old is not None:
        ref, S = ref + old.double(), S + old.double().abs()
    return ref, S


def modbank_fwd(lat, W, b, scale):
    """s[b,c] = scale sum_k lat[b,k] W[c,k] + bias[c]   (lat: the layer's latent rows [B, K])"""
    ref = scale * lat.double() @ W.double().t()
    S = scale * lat.double().abs() @ W.double().abs().t()
    if b is not None:
        ref, S = ref + b.double(), S + b.double().abs()
    return ref, S


def modbank_bwd(lat, gs, scale, old_w=None, old_b=None):
    """gW[c,k] (+)= scale sum_b gs[b,c] lat[b,k];  gb[c] (+)= sum_b gs[b,c] -> ((gW, S), (gb, S))"""
    gw, Sw = scale * gs.double().t() @ lat.double(), scale * gs.double().abs().t() @ lat.double().abs()
    gb, Sb = gs.double().sum(0), gs.double().abs().sum(0)
    if old_w is not None:
        gw, Sw = gw + old_w.double(), Sw + old_w.double().abs()
    if old_b is not None:
        gb, Sb = gb + old_b.double(), Sb + old_b.double().abs()
    return (gw, Sw), (gb, Sb)


def pixelnorm(x, eps):
    """x'[b,:] = x[b,:] rsqrt(mean_k x[b,k]^2 + eps)"""
    xd = x.double()
    return xd * ((xd ** 2).mean(1, keepdim=True) + eps) ** -0.5


def equal_linear(x, W, bias, scale, bias_mul, act, slope, gain, pn_eps=None):
    """out[b,o] = act(scale sum_k x'[b,k] W[o,k] + bias[o] bias_mul), act = gain * leaky_relu(., slope) or the identity;
    x' = pixelnorm(x) when pn_eps is given.  S carries the gain."""
    xd = x.double() if pn_eps is None else pixelnorm(x, pn_eps)
    pre, S = scale * xd @ W.double().t(), scale * xd.abs() @ W.double().abs().t()
    if bias is not None:
        pre, S = pre + bias.double() * bias_mul, S + bias.double().abs() * bias_mul
    if act:
        return torch.where(pre > 0, pre, pre * slope) * gain, S * gain
    return pre, S


def linear_fwd(x, W, bias, alpha, bias_mul):
    """out[b,o] = alpha sum_k x[b,k] W[o,k] + bias_mul bias[o]"""
    return equal_linear(x, W, bias, alpha, bias_mul, 0, 1.0, 1.0)


def linear_dgrad(g, W, alpha):
    """out[b,k] = alpha sum_o g[b,o] W[o,k]"""
    return alpha * g.double() @ W.double(), alpha * g.double().abs() @ W.double().abs()


def linear_wgrad(g, x, alpha, bias_mul, old_w=None, old_b=None):
    """gw[o,k] (+)= alpha sum_b g[b,o] x[b,k];  gb[o] (+)= bias_mul sum_b g[b,o] -> ((gw, S), (gb, S))"""
    gw, Sw = alpha * g.double().t() @ x.double(), alpha * g.double().abs().t() @ x.double().abs()
    gb, Sb = bias_mul * g.double().sum(0), bias_mul * g.double().abs().sum(0)
    if old_w is not None:
        gw, Sw = gw + old_w.double(), Sw + old_w.double().abs()
    if old_b is not None:
        gb, Sb = gb + old_b.double(), Sb + old_b.double().abs()
    return (gw, Sw), (gb, Sb)
