"""Singular-value adaptation (rick_amd/svd.py) restated in NumPy fp64: the two formulas as literal loops.  Nothing is imported
from rick_amd.svd.  Arrays: W0, G [co, ci, taps]; U [taps, co, r]; Vt [taps, r, ci]; d [taps, r].

    W^[o,i,t] = W0[o,i,t] + sum_k U[t,o,k] d[t,k] Vt[t,k,i]
    dd[t,k]   = sum_o sum_i U[t,o,k] G[o,i,t] Vt[t,k,i]

`apply_loops` / `grad_loops` are the four nested loops over t, o, i, k, one scalar at a time — the definition itself, usable up
to a few thousand elements.  `apply` / `grad` keep the loops over t and k and let NumPy's elementwise broadcast run the o and i
loops (an outer product per (t, k), added in ascending k; an elementwise triple product summed per (t, k)): the same terms in
fp64, no einsum, no matrix product — tests/test_svd.py holds the two forms together."""
import numpy as np


def _f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def apply_loops(w0, u, vt, d):
    w0, u, vt, d = _f64(w0, u, vt, d)
    co, ci, taps = w0.shape
    r = d.shape[1]
    out = w0.copy()
    for t in range(taps):
        for o in range(co):
            for i in range(ci):
                acc = 0.0
                for k in range(r):
                    acc += u[t, o, k] * d[t, k] * vt[t, k, i]
                out[o, i, t] = w0[o, i, t] + acc
    return out


def grad_loops(g, u, vt):
    g, u, vt = _f64(g, u, vt)
    co, ci, taps = g.shape
    r = u.shape[2]
    out = np.zeros((taps, r))
    for t in range(taps):
        for o in range(co):
            for i in range(ci):
                for k in range(r):
                    out[t, k] += u[t, o, k] * g[o, i, t] * vt[t, k, i]
    return out


def apply(w0, u, vt, d):
    w0, u, vt, d = _f64(w0, u, vt, d)
    co, ci, taps = w0.shape
    out = np.empty_like(w0)
    acc, term = np.empty((co, ci)), np.empty((co, ci))
    for t in range(taps):
        acc[:] = 0.0
        for k in range(d.shape[1]):
            np.multiply((u[t, :, k] * d[t, k])[:, None], vt[t, k, :][None, :], out=term)
            acc += term
        out[:, :, t] = w0[:, :, t] + acc
    return out


def grad(g, u, vt):
    g, u, vt = _f64(g, u, vt)
    taps, r = u.shape[0], u.shape[2]
    out = np.zeros((taps, r))
    term = np.empty(g.shape[:2])
    for t in range(taps):
        gt = np.ascontiguousarray(g[:, :, t])
        ut = np.ascontiguousarray(u[t].T)                      # [r, co]: row k is U[t, :, k]
        for k in range(r):
            np.multiply(gt, vt[t, k, :][None, :], out=term)
            term *= ut[k][:, None]
            out[t, k] = term.sum()
    return out
