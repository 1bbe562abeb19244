"""Dense numpy statement of the QP adjoint (include/mpcqp.h, mpcqp_adjoint_device) -- a helper
for tests/test_adjoint_ref.py (which checks it against finite differences of oracle solves) and
tests/test_adjoint_device.py (which checks the device kernel against it).  Not a test.

For one instance, in the caller's units, with z = A x:
  classes: 3 equality (l == u), 1 lower (z - l < -y), 2 upper (u - z < y), 0 inactive;
  K = [[P, A_act'], [A_act, 0]] over the active rows, K [r_x; r_y] = [g_x; g_y] (g_y on the
  active rows; r_y = 0 elsewhere);
  gq = -r_x; gl / gu = r_y on a lower / upper row, on an equality row to gl when y <= 0 and to
  gu when y > 0, zero where the bound is infinite; gA_ij = -(y_i r_x,j + r_y,i x_j);
  gP_ij = -(r_x,i x_j + r_x,j x_i) for i < j, gP_ii = -r_x,i x_i.
"""
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp

INFTY = 1e30


def full_P(P):
    """The symmetric matrix of an upper-triangular (or already symmetric) P, dense."""
    P = sp.csc_matrix(P)
    if abs(sp.tril(P, -1)).sum() == 0:
        P = sp.triu(P) + sp.triu(P, 1).T
    return np.asarray(P.todense(), float)


def row_classes(A, l, u, x, y, z=None):
    z = A @ x if z is None else z
    lower = z - l < -y
    upper = u - z < y
    return np.where(l == u, 3, np.where(lower, 1, np.where(upper, 2, 0))).astype(np.int8)


def kkt(P, A, act):
    Pd = full_P(P)
    Aa = np.asarray(sp.csc_matrix(A).todense(), float)[act != 0]
    k = Aa.shape[0]
    return np.block([[Pd, Aa.T], [Aa, np.zeros((k, k))]])


def adjoint(P, A, l, u, x, y, gx=None, gy=None, act=None, z=None):
    """Row classes, r_x, r_y and the five gradients for one seed (gx (n,), gy (m,)) or several
    ((nrhs, n), (nrhs, m)); gP on triu(P)'s stored entries and gA on A's, in CSC order."""
    A = sp.csc_matrix(A)
    A.sort_indices()
    Pu = sp.triu(sp.csc_matrix(P), format="csc")
    Pu.sort_indices()
    m, n = A.shape
    act = row_classes(A, l, u, x, y, z) if act is None else act
    on = act != 0
    flat = (gx is None or np.ndim(gx) == 1) and (gy is None or np.ndim(gy) == 1)
    R = np.atleast_2d(gx if gx is not None else gy).shape[0]
    GX = np.zeros((R, n)) if gx is None else np.atleast_2d(np.asarray(gx, float))
    GY = np.zeros((R, m)) if gy is None else np.atleast_2d(np.asarray(gy, float))
    K = kkt(Pu, A, act)
    rhs = np.concatenate([GX, GY[:, on]], axis=1).T
    s = np.linalg.solve(K, rhs).T
    rx = s[:, :n]
    ry = np.zeros((R, m))
    ry[:, on] = s[:, n:]
    to_l = ((act == 1) | ((act == 3) & (y <= 0))) & (l > -INFTY)
    to_u = ((act == 2) | ((act == 3) & (y > 0))) & (u < INFTY)
    gl = np.where(to_l, ry, 0.0)
    gu = np.where(to_u, ry, 0.0)
    ai, aj = A.indices, np.repeat(np.arange(n), np.diff(A.indptr))
    gA = -(y[ai] * rx[:, aj] + ry[:, ai] * x[aj])
    pi, pj = Pu.indices, np.repeat(np.arange(n), np.diff(Pu.indptr))
    gP = -(rx[:, pi] * x[pj] + rx[:, pj] * x[pi])
    gP = np.where(pi == pj, 0.5 * gP, gP)
    out = SimpleNamespace(act=act, rx=rx, ry=ry, gq=-rx, gl=gl, gu=gu, gPx=gP, gAx=gA, cond=np.linalg.cond(K))
    if flat:
        for k in ("rx", "ry", "gq", "gl", "gu", "gPx", "gAx"):
            setattr(out, k, getattr(out, k)[0])
    return out


def ruiz_scaling(P, q, A, scaling=10):
    """(D, E, c) of OSQP 0.6's scale_data (the restatement of tests/osqp_dense_ref.py): the
    solver works on P~ = c D P D, q~ = c D q, A~ = E A D."""
    lo, hi = 1e-4, 1e4

    def limit(v):
        v = np.where(v < lo, 1.0, v)
        return np.where(v > hi, hi, v)

    Pf, Ad, q = full_P(P), np.asarray(sp.csc_matrix(A).todense(), float), np.asarray(q, float).copy()
    n, m = Pf.shape[0], Ad.shape[0]
    D, E, c = np.ones(n), np.ones(m), 1.0
    for _ in range(scaling):
        Dt = np.maximum(np.abs(Pf).max(0), np.abs(Ad).max(0) if m else 0.0)
        Et = np.abs(Ad).max(1)
        Dt, Et = 1 / np.sqrt(limit(Dt)), 1 / np.sqrt(limit(Et))
        Pf, Ad, q = Dt[:, None] * Pf * Dt[None, :], Et[:, None] * Ad * Dt[None, :], Dt * q
        D, E = D * Dt, E * Et
        ct = max(np.abs(Pf).max(0).mean(), float(limit(np.array([np.abs(q).max()]))[0]))
        ct = 1 / float(limit(np.array([ct]))[0])
        Pf, q, c = Pf * ct, q * ct, c * ct
    return D, E, c


def residual(P, A, act, rx, ry, gx=None, gy=None, scaling=None):
    """||K s - g||_inf / max(||g||_inf, tiny) of a given (r_x, r_y), per seed (g_y and r_y count
    on the active rows only): on the unscaled system, or with scaling = (D, E, c) on the scaled
    one the device works on -- K~ of (c D P D, E A D), s~ = (r_x / (c D), r_y / E),
    g~ = (D g_x, E g_y / c) -- which is what the device's ares measures."""
    A = sp.csc_matrix(A)
    m, n = A.shape
    on = act != 0
    RX, RY = np.atleast_2d(rx), np.atleast_2d(ry)
    R = RX.shape[0]
    GX = np.zeros((R, n)) if gx is None else np.atleast_2d(np.asarray(gx, float))
    GY = np.zeros((R, m)) if gy is None else np.atleast_2d(np.asarray(gy, float))
    if scaling is not None:
        D, E, c = scaling
        P = c * (D[:, None] * full_P(P) * D[None, :])
        A = sp.csc_matrix(E[:, None] * np.asarray(A.todense(), float) * D[None, :])
        RX, RY, GX, GY = RX / (c * D), RY / E, GX * D, GY * E / c
    K = kkt(P, A, act)
    s = np.concatenate([RX, RY[:, on]], axis=1)
    g = np.concatenate([GX, GY[:, on]], axis=1)
    res = np.abs(s @ K.T - g).max(axis=1) / np.maximum(np.abs(g).max(axis=1), 1e-300)
    return res if np.ndim(rx) == 2 else res[0]


def rel_dev(a, b, floor=0.0):
    """max |a - b| / max(max |b|, floor, tiny): the relative deviation the tests bound.  `floor`
    keeps an array whose reference is zero or rounding noise (a gradient that vanishes) from
    being divided by nothing: the tests pass 1e-6 of the seed's largest reference array."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-300)) if b.size else 0.0
