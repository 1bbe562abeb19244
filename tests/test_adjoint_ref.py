"""The dense adjoint of tests/qp_adjoint_ref.py against central differences of oracle solves.

L = g_x . x of the oracle's polished solution (eps 1e-10) is differenced along random directions
in q, in l and u over the inequality rows, in l and u together over the equality rows, and in the
stored values of A and P (h = 1e-5), and compared with the helper's gradients contracted with
the same directions.  The solution map is piecewise affine, so every case first asserts that the
row classes are the same at the three evaluation points.

Tolerance: 1e-6 relative, 1e-5 for the A values (the polished solution is within 1e-8 of the
optimum -- the bar of test_polish_matches_oracle -- and the difference quotient divides what
the two solves do not share of that error by h = 1e-5).  Measured: <= 5e-8.  The quotient of
a derivative that is zero (an input at its bound does not move with q, A or P) is rounding
noise of the two solves over h, so a derivative below 1e-4 of the case's largest one is held to
that absolute level instead: the denominator is max(|fd|, 1e-4 * largest |fd| of the case).
"""
import numpy as np
import pytest
import scipy.sparse as sp

import pyoracle
import qp_adjoint_ref as ref
from osqp_amd import canonical_data, mpc
from test_oracle import osqp_demo_problem

H = 1e-5
SET = dict(eps_abs=1e-10, eps_rel=1e-10, max_iter=200000, polish=True, warm_start=False, verbose=False)


def _solve(P, q, A, l, u):
    o = pyoracle.OSQP()
    o.setup(P, q, A, l, u, **SET)
    r = o.solve()
    assert r.info.status == "solved"
    return r


def _demo():
    P, q, A, l, u = osqp_demo_problem()[:5]
    return P, q, A, l, u, 0


def _cfg2(i):
    b = mpc.make_batch(2, 4)
    P, A = b["P"].copy(), b["A"].copy()
    P.data, A.data = b["Px"][i].copy(), b["Ax"][i].copy()
    return P, b["q"][i], A, b["l"][i], b["u"][i], b["u_slice"].start


def _ltv(golden):
    g = golden("dyn_ltv_n30.npz")
    P, A = g["P"].copy(), g["A"].copy()
    q, l, u = g["q"], g["l"], g["u"]
    if q.ndim == 2:
        if "Px" in g:
            P.data, A.data = g["Px"][0].copy(), g["Ax"][0].copy()
        q, l, u = q[0], l[0], u[0]
    return P, q, A, l, u, 31 * 6  # the first input of the horizon (x_0..x_30 of 6 states, then u)


CASES = {"demo": lambda golden: _demo(), "cfg2[0]": lambda golden: _cfg2(0), "cfg2[1]": lambda golden: _cfg2(1),
         "dyn_ltv_n30": _ltv}


@pytest.mark.parametrize("name", list(CASES))
def test_dense_adjoint_matches_finite_differences(golden, name):
    P, q, A, l, u, idx = CASES[name](golden)
    P, A = canonical_data(P, A)
    l, u = np.maximum(l, -1e30), np.minimum(u, 1e30)
    n, m = P.shape[0], A.shape[0]
    r0 = _solve(P, q, A, l, u)
    rng = np.random.default_rng(0)
    gx = np.stack([np.zeros(n), rng.standard_normal(n)])  # e_idx (one input of the MPC cases) and a dense seed
    gx[0, idx] = 1.0
    a = ref.adjoint(P, A, l, u, r0.x, r0.y, gx)
    if name == "cfg2[1]":
        assert ((a.act == 1) | (a.act == 2)).any()  # the case with an active inequality
    eq = l == u
    fin_l, fin_u = l > -1e30, u < 1e30

    def fd(name_, **kw):
        d = dict(P=P, q=q, A=A, l=l, u=u)
        vals = []
        for sgn in (1.0, -1.0):
            e = dict(d)
            for k, dv in kw.items():
                if k in ("P", "A"):
                    M = d[k].copy()
                    M.data = d[k].data + sgn * H * dv
                    e[k] = M
                else:
                    e[k] = d[k] + sgn * H * dv
            r = _solve(e["P"], e["q"], e["A"], e["l"], e["u"])
            cls = ref.row_classes(e["A"], e["l"], e["u"], r.x, r.y)
            assert np.array_equal(cls, a.act), f"{name_}: the active set changes within the step"
            vals.append(gx @ r.x)
        return (vals[0] - vals[1]) / (2 * H)

    dq = rng.standard_normal(n)
    dl = rng.standard_normal(m) * (~eq & fin_l)
    du = rng.standard_normal(m) * (~eq & fin_u)
    de = rng.standard_normal(m) * eq
    dA = rng.standard_normal(A.nnz)
    dP = rng.standard_normal(P.nnz)
    checks = [
        ("q", fd("q", q=dq), a.gq @ dq, 1e-6),
        ("l", fd("l", l=dl), a.gl @ dl, 1e-6),
        ("u", fd("u", u=du), a.gu @ du, 1e-6),
        ("l+u (equality rows)", fd("l+u", l=de, u=de), (a.gl + a.gu) @ de, 1e-6),
        ("A values", fd("A", A=dA), a.gAx @ dA, 1e-5),
        ("P values", fd("P", P=dP), a.gPx @ dP, 1e-6),
    ]
    scale = np.max([np.abs(v) for _, v, _, _ in checks], axis=0)  # per seed
    for what, nums, anas, tol in checks:
        for k, (num, ana) in enumerate(zip(nums, anas)):
            err = abs(num - ana) / max(abs(num), 1e-4 * scale[k])
            print(f"{name} seed {k} {what}: fd {num:+.10e} adjoint {ana:+.10e} rel {err:.1e}")
            assert err < tol, (what, k, num, ana)


def test_residual_helper_is_zero_at_the_solution_and_sees_an_error():
    P, q, A, l, u = osqp_demo_problem()[:5]
    P, A = canonical_data(P, A)
    r = _solve(P, q, A, l, u)
    gx, gy = np.array([1.0, -2.0]), np.array([0.5, 0.0, 1.5])
    a = ref.adjoint(P, A, l, u, r.x, r.y, gx, gy)
    assert a.act.tolist() == [3, 0, 2]
    assert ref.residual(P, A, a.act, a.rx, a.ry, gx, gy) < 1e-14
    assert ref.residual(P, A, a.act, a.rx * (1 + 1e-3), a.ry, gx, gy) > 1e-5
    # a seed on an inactive row is ignored, r_y is zero there
    gy2 = gy + np.array([0.0, 7.0, 0.0])
    a2 = ref.adjoint(P, A, l, u, r.x, r.y, gx, gy2)
    assert np.array_equal(a2.rx, a.rx) and a2.ry[1] == 0.0
