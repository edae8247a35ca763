"""Kernel modulation (rick_amd/kml.py) in NumPy fp64: the four formulas and their error bounds.  Nothing is imported from
rick_amd.kml.  Arrays: W0, G [co, ci, taps]; a [co, R]; b [ci, R]; rows bool [co].

    s[o,i]    = sum_r a[o,r] b[i,r]
    W^[o,i,t] = W0[o,i,t] (1 + s[o,i])                 on rows[o]
    P[o,i]    = sum_t G[o,i,t] W0[o,i,t]
    da[o,r]   = sum_i P[o,i] b[i,r]                    (0 off rows)
    db[i,r]   = sum_{o in rows} P[o,i] a[o,r]

Bounds, u = 2^-24 (fp32 operands are exact in fp64; the fp64 evaluation's own error is below 2^-29 of these bounds):
    W^      : (R + 3) u |W0| (1 + sum_r |a b|): R products and R - 1 additions of s (gamma_R sum |a b|), the addition of 1, the product
              with W0, and one u of slack for the second-order terms.
    da, db  : (K + R + 4) u sum |terms|, the sum over the absolute values of every product G W0 b (G W0 a) entering the element;
              K = ci taps for da, K = taps x (flagged rows) for db.  A sum of K products of three factors, each product formed with
              two roundings, in ANY order of summation, errs by at most gamma_(K + 1) sum |terms|: the bound does not dictate the
              kernel's blocking.
"""
import numpy as np

U32 = 2.0 ** -24


def _f64(*xs):
    return [np.asarray(x, dtype=np.float64) for x in xs]


def s(a, b):
    a, b = _f64(a, b)
    return a @ b.T


def apply(w0, a, b):
    """W^ for every row, [co, ci, taps] fp64 (the caller keeps the rows it flags)."""
    (w0,) = _f64(w0)
    return w0 * (1.0 + s(a, b))[:, :, None]


def apply_bound(w0, a, b):
    w0, a, b = _f64(w0, a, b)
    R = a.shape[1]
    return (R + 3) * U32 * np.abs(w0) * (1.0 + np.abs(a) @ np.abs(b).T)[:, :, None]


def p(g, w0):
    g, w0 = _f64(g, w0)
    return (g * w0).sum(2)


def grads(g, w0, a, b, rows):
    """(da [co, R], db [ci, R]) in fp64."""
    a, b = _f64(a, b)
    rows = np.asarray(rows, dtype=bool)
    P = p(g, w0) * rows[:, None]
    return P @ b, P.T @ a


def grad_bounds(g, w0, a, b, rows):
    """(bound of da [co, R], bound of db [ci, R])."""
    g, w0, a, b = _f64(g, w0, a, b)
    rows = np.asarray(rows, dtype=bool)
    co, ci, taps = w0.shape
    R = a.shape[1]
    A = np.abs(g * w0).sum(2) * rows[:, None]                  # sum_t |G W0|, [co, ci]
    da = (ci * taps + R + 4) * U32 * (A @ np.abs(b))
    db = (taps * int(rows.sum()) + R + 4) * U32 * (A.T @ np.abs(a))
    return da, db
