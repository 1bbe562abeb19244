"""The numpy restatements of the MPC-step VJPs (osqp_amd.mpc.ltv_qp_vjp, incremental_qp_vjp,
linearise_kinematics_vjp, mpc_device.AffineMap.vjp) against central differences of the host
builders, and the whole chain linearise -> assemble -> solve against central differences of oracle
solves re-linearised at the moved state.  DESIGN.md §15 has the measured figures behind each bar.

The builders are linear in (Ad, Bd, gd, x0, Xr, xlo, xhi) and bilinear in (Q, Xr), so a central
difference with a step of order 1 is exact up to rounding: BAR_LINEAR is ten times the largest
deviation measured.  The linearisation is differenced with h = 1e-6 (BAR_LIN likewise).  The chain
takes h and its bar from tests/test_adjoint_ref.py: h = 1e-5, 1e-5 relative (the bar of that file's
A values -- the moved state reaches the solution through A's values), a derivative below 1e-4 of the
case's largest one being held to that absolute level.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import pyoracle
import qp_adjoint_ref as ref
from osqp_amd import canonical_data, mpc
from osqp_amd.mpc_device import AffineMap, lateral_builder

BAR_LINEAR = 1.5e-13   # measured <= 1.43e-14 of the contraction's largest term (nx 1, N 3: R +- its step)
BAR_LIN = 1e-7         # measured <= 9.99e-9 of the sample's largest gradient (h = 1e-6: eps / h of the quotient)
H = 1e-5
BAR_CHAIN = 1e-5
H_Q = 1e-3             # the step in a weight: they are 10 .. 1000 and d u_0 / d Q ~ 1e-6, which at h = 1e-5
                       # is the rounding of two solves over h (measured with 1e-3: <= 1.1e-6)
SET = dict(eps_abs=1e-10, eps_rel=1e-10, max_iter=200000, polish=True, warm_start=False, verbose=False)
LF, LR, DT = 1.25, 1.40, 0.02

LAYOUTS = {
    "kin": (4, 2, mpc.KIN_MASK_A, mpc.KIN_MASK_B),
    "dyn": (6, 2, mpc.DYN_MASK_A, mpc.DYN_MASK_B),
    "one": (1, 1, np.ones((1, 1), np.uint8), np.ones((1, 1), np.uint8)),
}


def sym_weights(rng, nx, nu):
    """Non-diagonal symmetric Q, QN (tridiagonal: the corner pairs are not stored in P) and R."""
    def tri(k, full):
        M = np.diag(rng.uniform(5, 10, k))
        for i in range(k - 1):
            M[i, i + 1] = M[i + 1, i] = rng.uniform(0.5, 1.5)
        if full and k > 1:
            M[0, k - 1] = M[k - 1, 0] = rng.uniform(0.2, 0.4)
        return M
    return tri(nx, False), tri(nx, False), tri(nu, True)


def random_case(rng, kind, name, N):
    nx, nu, mA, mB = LAYOUTS[name]
    nxa = nx + nu if kind == "incr" else nx
    Q, QN, R = sym_weights(rng, nx, nu)
    d = dict(Ad=rng.standard_normal((N, nx, nx)) * mA, Bd=rng.standard_normal((N, nx, nu)) * mB,
             gd=rng.standard_normal((N, nx)), x0=rng.standard_normal(nxa), Xr=rng.standard_normal((nx, N + 1)),
             Q=Q, QN=QN, R=R)
    if kind == "ltv":
        xlo, xhi = -1 - rng.uniform(0, 1, (N + 1, nx)), 1 + rng.uniform(0, 1, (N + 1, nx))
        xlo[0, 0], xhi[1, 0], xhi[N, nx - 1] = -np.inf, np.inf, 2e30       # clipped by the forward
        d.update(xlo=xlo, xhi=xhi)
    return d, (nx, nu, nxa, mA, mB)


def build(kind, d, N, nx, nu):
    if kind == "ltv":
        out = mpc.ltv_qp(list(d["Ad"]), list(d["Bd"]), list(d["gd"]), d["x0"], d["Xr"], d["Q"], d["QN"], d["R"], N,
                         np.zeros(nx), np.zeros(nx), -np.ones(nu), np.ones(nu), xlo=d["xlo"], xhi=d["xhi"])
    else:
        out = mpc.incremental_qp(list(d["Ad"]), list(d["Bd"]), list(d["gd"]), d["x0"], d["Xr"], d["Q"], d["QN"],
                                 d["R"], N, -np.ones(nx + nu), np.ones(nx + nu), -np.ones(nu), np.ones(nu))
    P, q, A, l, u = out
    P = sp.triu(P, format="csc"); P.sort_indices()
    return P, q, A, np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30)


def vjp(kind, P, A, N, nx, nu, d, cot):
    if kind == "ltv":
        return mpc.ltv_qp_vjp(P, A, N, nx, nu, d["Q"], d["QN"], d["Xr"], xlo=d["xlo"], xhi=d["xhi"], **cot)
    return mpc.incremental_qp_vjp(P, A, N, nx, nu, d["Q"], d["QN"], d["Xr"], **cot)


@pytest.mark.parametrize("N", [2, 3])
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["ltv", "incr"])
def test_assembly_vjp_matches_central_differences(kind, name, N):
    rng = np.random.default_rng(7 + N)
    d, (nx, nu, nxa, mA, mB) = random_case(rng, kind, name, N)
    P, q, A, l, u = build(kind, d, N, nx, nu)
    cot = dict(gPx=rng.standard_normal(P.nnz), gAx=rng.standard_normal(A.nnz), gq=rng.standard_normal(q.size),
               gl=rng.standard_normal(l.size), gu=rng.standard_normal(u.size))
    g = vjp(kind, P, A, N, nx, nu, d, cot)
    grads = dict(Ad=g.gAd, Bd=g.gBd, gd=g.ggd, x0=g.gx0, Xr=g.gXr, Q=g.gQ, QN=g.gQN, R=g.gR)
    if kind == "ltv":
        grads.update(xlo=g.gxlo, xhi=g.gxhi)
        assert g.gxlo[0, 0] == 0 and g.gxhi[1, 0] == 0 and g.gxhi[N, nx - 1] == 0 and g.gxlo[1, 0] != 0
    assert not g.gAd[:, mA == 0].any() and not g.gBd[:, mB == 0].any()
    assert g.gAd[:, mA != 0].all() and g.gBd[:, mB != 0].all()
    # entries of the weights P does not store (the lower triangle; the corner pair, zero at creation)
    stored = {"Q": np.triu(d["Q"] != 0), "QN": np.triu(d["QN"] != 0), "R": np.triu(d["R"] != 0)}
    worst = 0.0
    for key, grad in grads.items():
        dirn = rng.standard_normal(np.shape(d[key]))
        if key in ("Ad", "Bd"):
            dirn = dirn * (mA if key == "Ad" else mB)
        if key in stored:   # keep the builder's P pattern: no step on an upper entry that is not stored
            dirn = np.where(np.triu(np.ones_like(dirn, bool)) & ~stored[key], 0.0, dirn)
        if key in ("xlo", "xhi"):
            dirn = np.where(np.isfinite(d[key]), dirn, 0.0)
        outs = []
        for sgn in (1.0, -1.0):
            e = dict(d)
            e[key] = d[key] + sgn * dirn
            Pe, qe, Ae, le, ue = build(kind, e, N, nx, nu)
            assert np.array_equal(Pe.indices, P.indices) and np.array_equal(Ae.indices, A.indices)
            outs.append((Pe.data, Ae.data, qe, le, ue))
        terms = []
        for c, vp_, vm in zip((cot["gPx"], cot["gAx"], cot["gq"], cot["gl"], cot["gu"]), *outs):
            diff = np.where(vp_ == vm, 0.0, (vp_ - vm) / 2.0)     # (a clipped bound is 1e30 on both sides)
            terms.append(c * diff)
        terms = np.concatenate(terms)
        fd, an = terms.sum(), float(np.sum(grad * dirn))
        dev = abs(fd - an) / max(np.abs(terms).max(), 1e-300)
        worst = max(worst, dev)
        print(f"{kind} {name} N={N} {key}: fd {fd:+.12e} vjp {an:+.12e} deviation {dev:.1e}")
        assert np.abs(terms).max() > 0, key
        assert dev < BAR_LINEAR, (key, fd, an)
    print(f"{kind} {name} N={N}: worst deviation {worst:.2e}")


def test_incremental_doubled_bd_slot():
    """Bd_k sits twice in the incremental layout's A: a cotangent on one slot alone, on the other
    alone and on both must each arrive."""
    N, (nx, nu, mA, mB) = 2, LAYOUTS["kin"]
    rng = np.random.default_rng(1)
    d, _ = random_case(rng, "incr", "kin", N)
    P, q, A, l, u = build("incr", d, N, nx, nu)
    nxa, ns = nx + nu, (N + 1) * (nx + nu)
    i, j = np.argwhere(mB != 0)[0]
    for k in range(N):
        s_aug = mpc._slots(A, [(k + 1) * nxa + i], [k * nxa + nx + j])[0]
        s_b = mpc._slots(A, [(k + 1) * nxa + i], [ns + k * nu + j])[0]
        assert s_aug >= 0 and s_b >= 0 and s_aug < s_b
        for slots, expect in (((s_aug,), 2.0), ((s_b,), 3.0), ((s_aug, s_b), 5.0)):
            gAx = np.zeros(A.nnz)
            for s in slots:
                gAx[s] = 2.0 if s == s_aug else 3.0
            g = mpc.incremental_qp_vjp(P, A, N, nx, nu, d["Q"], d["QN"], gAx=gAx)
            want = np.zeros((N, nx, nu))
            want[k, i, j] = expect
            assert np.array_equal(g.gBd, want) and not g.gAd.any()


def test_kin_linearise_vjp_matches_central_differences():
    rng = np.random.default_rng(5)
    n, h = 64, 1e-6
    x = np.stack([rng.standard_normal(n), rng.standard_normal(n), rng.uniform(2, 12, n), rng.uniform(-1, 1, n)], 1)
    u = np.stack([rng.uniform(-0.25, 0.25, n), rng.uniform(-1, 1, n)], 1)
    gAd, gBd, ggd = rng.standard_normal((n, 4, 4)), rng.standard_normal((n, 4, 2)), rng.standard_normal((n, 4))
    gx, gu = mpc.linearise_kinematics_vjp(LF, LR, DT, x, u, gAd, gBd, ggd)
    assert not gx[:, :2].any() and not gu[:, 1].any()

    def loss(x_, u_):
        Ad, Bd, gd = mpc.linearise_kinematics(LF, LR, DT, x_, u_)
        return (gAd * Ad).sum((1, 2)) + (gBd * Bd).sum((1, 2)) + (ggd * gd).sum(1)

    worst = 0.0
    for arr, grad, cols in ((x, gx, range(4)), (u, gu, range(2))):
        for c in cols:
            e = np.zeros_like(arr)
            e[:, c] = h
            fd = (loss(x + e, u) - loss(x - e, u)) / (2 * h) if arr is x else (loss(x, u + e) - loss(x, u - e)) / (2 * h)
            scale = np.abs(np.concatenate([gx, gu], 1)).max(1)
            dev = (np.abs(fd - grad[:, c]) / scale).max()
            worst = max(worst, dev)
            print(f"linearise vjp {'x' if arr is x else 'u'}[{c}]: deviation {dev:.2e}")
            assert dev < BAR_LIN
    print(f"linearise vjp: worst deviation {worst:.2e}")


def test_affine_map_vjp_is_the_transpose():
    build_, nparam, nreg, _ = lateral_builder("vanilla", 3)
    amap = AffineMap(build_, nparam, nreg)
    rng = np.random.default_rng(2)
    E = np.concatenate([np.zeros((1, nparam)), np.eye(nparam)])
    ev = np.concatenate(amap.evaluate(E), axis=1)
    J = (ev[1:] - ev[:1]).T
    g = [rng.standard_normal((3, w)) for w in amap.seglen]
    got, want = amap.vjp(*g), np.concatenate(g, axis=1) @ J
    dev = np.abs(got - want).max() / np.abs(want).max()
    print(f"AffineMap.vjp against the probed Jacobian: deviation {dev:.2e}")
    assert dev < BAR_LINEAR
    assert np.array_equal(amap.vjp(g[0], None, None), amap.vjp(g[0], 0 * g[1], 0 * g[2]))


# ------------------------------------------------------------------ the whole chain --
def _solve(P, q, A, l, u):
    o = pyoracle.OSQP()
    o.setup(P, q, A, l, u, **SET)
    r = o.solve()
    assert r.info.status == "solved"
    return r


def ltv_reference(N):
    return np.stack([np.linspace(0.5, 0.5 + 0.2 * N, N + 1), np.zeros(N + 1), np.full(N + 1, 10.0), np.zeros(N + 1)])


def chain_problem(kind, N, x0, u0, x_lin=None, Q=None):
    """The QP of one MPC step with the model linearised at (x_lin, u0) on every stage (x_lin None:
    at x0 itself), canonical, bounds clipped."""
    x_lin = x0 if x_lin is None else x_lin
    Ad, Bd, gd = (v[0] for v in mpc.linearise_kinematics(LF, LR, DT, x_lin, u0))
    Xr = ltv_reference(N)
    if kind == "ltv":
        P, q, A, l, u = mpc.ltv_qp([Ad] * N, [Bd] * N, [gd] * N, x0, Xr, mpc.KINLTV_Q if Q is None else Q,
                                   mpc.KINLTV_QN, mpc.KINLTV_R, N, mpc.KINLTV_XMIN, mpc.KINLTV_XMAX, mpc.KINLTV_UMIN,
                                   mpc.KINLTV_UMAX)
    else:
        P, q, A, l, u = mpc.incremental_qp([Ad] * N, [Bd] * N, [gd] * N, np.concatenate([x0, u0]), Xr,
                                           mpc.KIN_Q if Q is None else Q, mpc.KIN_QN, mpc.KIN_R, N, mpc.KIN_XMIN_T,
                                           mpc.KIN_XMAX_T, mpc.KIN_DUMIN, -mpc.KIN_DUMIN)
    P, A = canonical_data(P, A)
    return P, q, A, np.maximum(l, -1e30), np.minimum(u, 1e30), Xr


def chain_gradients(kind, N, x0, u0, P, A, l, u, x, y, seed, Q):
    """(frozen gain, total gain, gQ) of L = seed . x: adjoint -> assembly VJP -> linearisation VJP
    of every stage (all linearised at (x0, u0): the stage sum)."""
    a = ref.adjoint(P, A, l, u, x, y, seed)
    fn = mpc.ltv_qp_vjp if kind == "ltv" else mpc.incremental_qp_vjp
    g = fn(P, A, N, 4, 2, Q, mpc.KINLTV_QN if kind == "ltv" else mpc.KIN_QN, ltv_reference(N), gPx=a.gPx, gAx=a.gAx, gq=a.gq, gl=a.gl, gu=a.gu)
    gx, _ = mpc.linearise_kinematics_vjp(LF, LR, DT, np.tile(x0, (N, 1)), np.tile(u0, (N, 1)), g.gAd, g.gBd, g.ggd)
    return a, g.gx0[:4].copy(), g.gx0[:4] + gx.sum(0), g.gQ


def run_chain(kind, N, x0, u0, seed_index, label):
    Q = mpc.KINLTV_Q if kind == "ltv" else mpc.KIN_Q
    P, q, A, l, u, Xr = chain_problem(kind, N, x0, u0)
    r0 = _solve(P, q, A, l, u)
    seed = np.zeros(P.shape[0])
    seed[seed_index] = 1.0
    a, frozen, total, gQ = chain_gradients(kind, N, x0, u0, P, A, l, u, r0.x, r0.y, seed, Q)

    def value(xm, x_lin=None, Qm=None):
        Pm, qm, Am, lm, um, _ = chain_problem(kind, N, xm, u0, x_lin, Qm)
        r = _solve(Pm, qm, Am, lm, um)
        cls = ref.row_classes(Am, lm, um, r.x, r.y)
        assert np.array_equal(cls, a.act), f"{label}: the active set changes within the step"
        return r.x[seed_index]

    fd_total = np.array([(value(x0 + H * e) - value(x0 - H * e)) / (2 * H) for e in np.eye(4)])
    fd_frozen = np.array([(value(x0 + H * e, x0) - value(x0 - H * e, x0)) / (2 * H) for e in np.eye(4)])
    fd_Q = np.array([(value(x0, None, Q + H_Q * np.diag(e)) - value(x0, None, Q - H_Q * np.diag(e))) / (2 * H_Q)
                     for e in np.eye(4)])
    out = dict(a=a, frozen=frozen, total=total, fd_total=fd_total, r0=r0)
    for what, fd, an in (("frozen", fd_frozen, frozen), ("total", fd_total, total), ("Q diagonal", fd_Q, np.diag(gQ))):
        den = np.maximum(np.abs(fd), 1e-4 * np.abs(fd).max())
        dev = np.abs(fd - an) / den
        print(f"{label} {what}: fd {fd} chain {an} deviation {dev.max():.1e}")
        assert (dev < BAR_CHAIN).all(), (what, fd, an)
    return out


X0_LTV, U0_LTV = np.array([0.3, 0.2, 8.0, 0.05]), np.array([0.02, 0.1])


@pytest.mark.parametrize("N", [2, 3, 5])
def test_ltv_chain_matches_relinearised_differences(N):
    o = run_chain("ltv", N, X0_LTV, U0_LTV, (N + 1) * 4, f"kin ltv N={N}")
    act = o["a"].act
    assert not ((act == 1) | (act == 2)).any()                 # no inequality is active
    # the linearisation term is not small: dropping it must not pass
    gap = np.abs(o["total"] - o["frozen"])
    floor = BAR_CHAIN * np.abs(o["fd_total"]).max()
    print(f"kin ltv N={N}: total - frozen {o['total'] - o['frozen']}, bar {floor:.1e}")
    assert gap[2] > 100 * floor and gap[3] > 100 * floor
    if N == 3:   # the oracle's figures of the issue this answers
        assert np.allclose(o["frozen"], [1.0136e-4, -2.0256e-3, -3.13e-6, -8.198e-3], rtol=2e-3)
        assert np.allclose(o["total"], [1.0136e-4, -2.0256e-3, -1.66e-4, -8.821e-3], rtol=4e-3)


INCR_CASES = {
    "interior steer": (np.array([0.3, 0.002, 9.9, 0.0005]), np.array([0.001, 0.0]), 0, False),
    "interior accel": (np.array([0.3, 0.002, 9.9, 0.0005]), np.array([0.001, 0.0]), 1, False),
    "active accel": (np.array([0.3, 0.2, 8.0, 0.05]), np.array([0.02, 0.1]), 1, True),
}


@pytest.mark.parametrize("case", list(INCR_CASES))
def test_incremental_chain_matches_relinearised_differences(case):
    x0, u0, j, active = INCR_CASES[case]
    N = 3
    o = run_chain("incr", N, x0, u0, (N + 1) * 6 + j, f"kin incr {case}")
    act, y = o["a"].act, o["r0"].y
    rows = 2 * (N + 1) * 6 + 2 * np.arange(N)                   # the steer-increment rows of the box
    if active:
        assert np.isin(act[rows], (1, 2)).any() and np.abs(y[rows[np.isin(act[rows], (1, 2))]]).min() >= 2.0
    else:
        assert not ((act == 1) | (act == 2)).any()
        du0 = o["r0"].x[(N + 1) * 6:(N + 1) * 6 + 2]
        assert np.all(np.abs(du0) < -mpc.KIN_DUMIN)
