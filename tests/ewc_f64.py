"""The elastic-weight-consolidation penalty in NumPy fp64: value, gradient term, mask rule and the two error bounds.  Nothing is
imported from rick_amd.ewc.

    kept     : the elements i with (mask[i] & 3) == 0 (all of them without a mask)
    value    : sum over kept of F_i d_i^2, d_i = fl32(theta_i - theta*_i) — the difference as the definition forms it, in fp32;
               every product in fp64, added without further rounding error (math.fsum)
    gradient : 2 weight F_i (theta_i - theta*_i) on kept, 0 elsewhere — exact operands, fp64 throughout
"""
import math

import numpy as np

U32 = 2.0 ** -24      # unit roundoff of fp32
U64 = 2.0 ** -53


def kept(mask, n):
    return np.ones(n, dtype=bool) if mask is None else (np.asarray(mask).astype(np.uint8) & 3) == 0


def value(theta, anchor, fisher, mask=None):
    theta, anchor = np.asarray(theta, dtype=np.float32), np.asarray(anchor, dtype=np.float32)
    d = (theta - anchor).astype(np.float64)
    terms = np.asarray(fisher, dtype=np.float64) * d * d
    return math.fsum(terms[kept(mask, theta.size)].tolist())


def grad_term(theta, anchor, fisher, weight, mask=None):
    theta = np.asarray(theta, dtype=np.float64)
    t = 2.0 * float(weight) * np.asarray(fisher, dtype=np.float64) * (theta - np.asarray(anchor, dtype=np.float64))
    return np.where(kept(mask, theta.size), t, 0.0)


def grad_bound(g0, term):
    """|g_dev - (g0 + term)| per element: three fp32 roundings — the difference, the product and the FMA."""
    return 3 * U32 * (np.abs(np.asarray(g0, dtype=np.float64)) + np.abs(term))


def value_bound(n, v):
    """|v_dev - v|: n non-negative fp64 terms, each rounded once and each passing through fewer than n additions."""
    return n * 2 * U64 * v
