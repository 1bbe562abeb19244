"""osqp_amd.mpc.linearise_dynamics_vjp, the numpy statement of k_linearise_vjp:
against central differences of mpc.linearise_dynamics on both signs of vx and inside the low-speed
guard, and as the last link of the whole chain linearise -> assemble -> solve on the dynamic
bicycle, against central differences of oracle solves re-linearised at the moved state.

The chain's helpers, step and bar are those of tests/test_mpc_vjp_ref.py (H = 1e-5, BAR_CHAIN =
1e-5 with its floor rule); tests/test_dyn_vjp_device.py evaluates the same chain at the device's
solution.
"""
import numpy as np
import pytest

import qp_adjoint_ref as ref
import test_mpc_vjp_ref as cpu
from osqp_amd import canonical_data, mpc

VEH = mpc.VehicleParams()
H_LIN = 1e-6
# measured 6.36e-10 of the row's largest gradient (4.93e-10 on the rows with vx < 0), the quotient
# taken as central_differences takes it; ten times that
BAR_LIN = 6.4e-9
# Inside the guard the tyre angles are 0 and what still carries derivative is smooth, while a row's
# largest gradient falls to dt |cotangent| ~ 0.02 (two or three entries of Bd and gd move at all), so
# the rounding of the forward's own entries, eps |accel| dt / h ~ 3e-11 per entry at h = 1e-6,
# counts thirty times more than outside.  The step there is 1e-5: the quotients at 1e-5 and 2e-5
# agree to 3.1e-9 of the same scale (asserted: the reference's own error, below the bar), at 1e-6
# they carry 3.1e-8 of rounding (measured deviation at 1e-5: 1.57e-9).
H_GUARD = 1e-5

# the two points of the chain (no entry of vy, r, steer is exactly 0: scipy would drop the entries
# of Ad that vanish there from the host builder's pattern)
X0_INTERIOR = np.array([0.3, 0.002, 0.0005, 9.9, 0.02, 0.01])
X0_ACTIVE = np.array([0.3, 0.2, 0.05, 9.9, 0.02, 0.01])
U0 = np.array([0.001, 0.0])
NX, NU, NXA = 6, 2, 8


def sample(rng, n):
    """X, Y in +-50, yaw in +-3, |vx| in [2, 15] with both signs, vy in +-1.5, r in +-0.6, steer in
    +-0.26, accel in [-3, 1]."""
    x = np.stack([rng.uniform(-50, 50, n), rng.uniform(-50, 50, n), rng.uniform(-3, 3, n),
                  rng.uniform(2, 15, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-1.5, 1.5, n),
                  rng.uniform(-0.6, 0.6, n)], -1)
    u = np.stack([rng.uniform(-0.26, 0.26, n), rng.uniform(-3, 1, n)], -1)
    return x, u


def guard_speeds(rng, n):
    """vx in +-0.49, at least 0.01 away from 0, +-0.3 and +-0.5: |vx| in [0.01, 0.29] or [0.31, 0.49]."""
    inner = rng.uniform(size=n) < 0.5
    mag = np.where(inner, rng.uniform(0.01, 0.29, n), rng.uniform(0.31, 0.49, n))
    return mag * rng.choice([-1.0, 1.0], n)


def cotangents(rng, lead):
    return rng.standard_normal(lead + (6, 6)), rng.standard_normal(lead + (6, 2)), rng.standard_normal(lead + (6,))


def central_differences(x, u, gAd, gBd, ggd, h):
    """Of the contraction of (Ad, Bd, gd) with the cotangents.  The outputs are differenced entry by
    entry before they are contracted, so that what does not move (Ad's unit diagonal, the zeros)
    leaves the quotient exactly and its rounding is that of the entries that do; the divisor is the
    step the two points really are apart (|x| eps / h of the nominal 2 h is 3e-9 at vx = 15)."""
    def quotient(xp, up, xm, um):
        p, m_ = mpc.linearise_dynamics(VEH, xp, up), mpc.linearise_dynamics(VEH, xm, um)
        step = (xp - xm).sum(1) + (up - um).sum(1)               # the step as it was rounded into the point
        return ((gAd * (p[0] - m_[0])).sum((1, 2)) + (gBd * (p[1] - m_[1])).sum((1, 2))
                + (ggd * (p[2] - m_[2])).sum(1)) / step

    fx, fu = np.zeros(x.shape), np.zeros(u.shape)
    for c in range(6):
        e = np.zeros(6)
        e[c] = h
        fx[:, c] = quotient(x + e, u, x - e, u)
    for c in range(2):
        e = np.zeros(2)
        e[c] = h
        fu[:, c] = quotient(x, u + e, x, u - e)
    return fx, fu


def _deviation(gx, gu, fx, fu):
    """test_kin_linearise_vjp_matches_central_differences's measure: over the largest gradient of the row"""
    g, f = np.concatenate([gx, gu], 1), np.concatenate([fx, fu], 1)
    return np.abs(f - g) / np.abs(g).max(1)[:, None]


def test_dyn_linearise_vjp_matches_central_differences():
    rng = np.random.default_rng(5)
    n = 64
    x, u = sample(rng, n)
    assert (x[:, 3] < 0).sum() >= 16 and (x[:, 3] > 0).sum() >= 16
    cots = cotangents(rng, (n,))
    gx, gu = mpc.linearise_dynamics_vjp(VEH, x, u, *cots)
    assert np.isfinite(gx).all() and np.isfinite(gu).all()
    assert not gx[:, :2].any()
    assert gx[:, 2:].all() and gu.all()                          # every other input carries derivative
    dev = _deviation(gx, gu, *central_differences(x, u, *cots, H_LIN))
    neg = x[:, 3] < 0
    print(f"dyn linearise vjp: largest gradient {max(np.abs(gx).max(), np.abs(gu).max()):.3g}, deviation per column "
          f"{dev.max(0)}, worst {dev.max():.2e} (vx < 0: {dev[neg].max():.2e}), bar {BAR_LIN:.1e}")
    assert dev.max() < BAR_LIN
    # None is a zero cotangent, and the three parts add up
    parts = [mpc.linearise_dynamics_vjp(VEH, x, u, *[c if i == k else None for i, c in enumerate(cots)])
             for k in range(3)]
    assert np.allclose(sum(p[0] for p in parts), gx, rtol=0, atol=1e-13 * np.abs(gx).max())
    assert np.allclose(sum(p[1] for p in parts), gu, rtol=0, atol=1e-13 * np.abs(gu).max())
    # leading axes are free
    g3 = mpc.linearise_dynamics_vjp(VEH, x.reshape(8, 8, 6), u.reshape(8, 8, 2), *[c.reshape((8, 8) + c.shape[1:])
                                                                                  for c in cots])
    assert np.array_equal(g3[0].reshape(n, 6), gx) and np.array_equal(g3[1].reshape(n, 2), gu)


def test_dyn_linearise_vjp_in_the_guard():
    rng = np.random.default_rng(6)
    n = 64
    x, u = sample(rng, n)
    x[:, 3] = guard_speeds(rng, n)
    low = np.abs(x[:, 3]) < 0.3
    assert low.sum() >= 8 and (~low).sum() >= 8 and (x[:, 3] < 0).sum() >= 8
    cots = cotangents(rng, (n,))
    gx, gu = mpc.linearise_dynamics_vjp(VEH, x, u, *cots)
    # the zero pattern, exactly: X, Y never; vy, r, steer not below 0.5; vx not below 0.3
    assert not gx[:, :2].any() and not gx[:, 4:].any() and not gu[:, 0].any()
    assert not gx[low, 3].any() and gx[~low, 3].all()
    assert gx[:, 2].all() and gu[:, 1].all()
    fd, fd2 = central_differences(x, u, *cots, H_GUARD), central_differences(x, u, *cots, 2 * H_GUARD)
    dev = _deviation(gx, gu, *fd)
    own = (np.abs(np.concatenate(fd2, 1) - np.concatenate(fd, 1)) / np.abs(np.concatenate([gx, gu], 1)).max(1)[:, None]
           ).max()
    print(f"dyn linearise vjp in the guard: deviation per column {dev.max(0)}, worst {dev.max():.2e}; the quotients "
          f"at h and 2 h differ by {own:.2e}")
    assert own < BAR_LIN
    assert dev.max() < BAR_LIN


# ------------------------------------------------------------------ the whole chain --
def dyn_reference(N):
    Xr = np.zeros((NX, N + 1))
    Xr[0] = np.linspace(0.5, 0.5 + 0.5 * N, N + 1)
    Xr[3] = 10.0
    return Xr


def chain_problem(N, x0, u0, x_lin=None, Q=None, Xr=None):
    """The QP of one incremental MPC step of DynamicMPC's weights and bounds with the dynamic
    bicycle linearised at (x_lin, u0) on every stage (x_lin None: at x0 itself), canonical, bounds
    clipped."""
    x_lin = x0 if x_lin is None else x_lin
    Ad, Bd, gd = (v[0] for v in mpc.linearise_dynamics(VEH, x_lin[None], u0[None]))
    Xr = dyn_reference(N) if Xr is None else Xr
    P, q, A, l, u = mpc.incremental_qp([Ad] * N, [Bd] * N, [gd] * N, np.concatenate([x0, u0]), Xr,
                                       mpc.DYN_Q if Q is None else Q, mpc.DYN_QN, mpc.DYN_R, N, mpc.DYN_XMIN_T,
                                       mpc.DYN_XMAX_T, mpc.DYN_DUMIN, -mpc.DYN_DUMIN)
    P, A = canonical_data(P, A)
    assert A.nnz == expected_nnz_A(N), "an entry of Ad / Bd is exactly 0 at this point: the host pattern lost it"
    return P, q, A, np.maximum(l, -1e30), np.minimum(u, 1e30), Xr


def expected_nnz_A(N):
    """A's entries with every structural nonzero of (Ad, Bd) present: -I, the stage blocks
    [[Ad, Bd], [0, I]] and [Bd; I], and the identity of the inequality rows."""
    nA, nB = int(mpc.DYN_MASK_A.sum()), int(mpc.DYN_MASK_B.sum())
    return (N + 1) * NXA + N * (nA + nB + NU) + N * (nB + NU) + (N + 1) * NXA + N * NU


def chain_gradients(N, x0, u0, P, A, l, u, x, y, seed, Q=None, Xr=None):
    """(adjoint, frozen gain, total gain, gQ) of L = seed . x in x0: adjoint -> assembly VJP ->
    linearise_dynamics_vjp of every stage (all linearised at (x0, u0): the stage sum)."""
    a = ref.adjoint(P, A, l, u, x, y, seed)
    g = mpc.incremental_qp_vjp(P, A, N, NX, NU, mpc.DYN_Q if Q is None else Q, mpc.DYN_QN,
                               dyn_reference(N) if Xr is None else Xr, gPx=a.gPx, gAx=a.gAx, gq=a.gq, gl=a.gl, gu=a.gu)
    gx, _ = mpc.linearise_dynamics_vjp(VEH, np.tile(x0, (N, 1)), np.tile(u0, (N, 1)), g.gAd, g.gBd, g.ggd)
    return a, g.gx0[:NX].copy(), g.gx0[:NX] + gx.sum(0), g.gQ


def steer_rows(N):
    """the steer-increment rows of the box, stage by stage"""
    return 2 * (N + 1) * NXA + NU * np.arange(N)


def run_chain(N, x0, u0, seed_index, label):
    P, q, A, l, u, _ = chain_problem(N, x0, u0)
    r0 = cpu._solve(P, q, A, l, u)
    seed = np.zeros(P.shape[0])
    seed[seed_index] = 1.0
    a, frozen, total, _ = chain_gradients(N, x0, u0, P, A, l, u, r0.x, r0.y, seed)

    def value(xm, x_lin=None):
        Pm, qm, Am, lm, um, _ = chain_problem(N, xm, u0, x_lin)
        r = cpu._solve(Pm, qm, Am, lm, um)
        cls = ref.row_classes(Am, lm, um, r.x, r.y)
        assert np.array_equal(cls, a.act), f"{label}: the active set changes within the step"
        return r.x[seed_index]

    Hs = cpu.H
    fd_total = np.array([(value(x0 + Hs * e) - value(x0 - Hs * e)) / (2 * Hs) for e in np.eye(NX)])
    fd_frozen = np.array([(value(x0 + Hs * e, x0) - value(x0 - Hs * e, x0)) / (2 * Hs) for e in np.eye(NX)])
    worst = 0.0
    for what, fd, an in (("frozen", fd_frozen, frozen), ("total", fd_total, total)):
        den = np.maximum(np.abs(fd), 1e-4 * np.abs(fd).max())
        dev = np.abs(fd - an) / np.where(den > 0, den, 1.0)      # (an all-zero quotient: absolute)
        worst = max(worst, dev.max())
        print(f"{label} {what}: fd {fd} chain {an} deviation {dev.max():.1e}")
        assert (dev < cpu.BAR_CHAIN).all(), (what, fd, an)
    return dict(a=a, frozen=frozen, total=total, fd_total=fd_total, r0=r0, worst=worst)


def seed_of(N, stage, j):
    return (N + 1) * NXA + stage * NU + j


CHAIN_CASES = {
    # the point, N, (stage, entry) of the increment that is the loss, the stages whose steer-increment
    # row is active (the oracle's: two box rows on the second point), and the entries of x0 in which
    # total - frozen is held above 100 bars (yaw, vy, r; with the accel seed on the interior point the
    # yaw entry's gap is 8.7e-5, seven bars, and is left out)
    "interior N=2 du0 steer": (X0_INTERIOR, 2, (0, 0), (), (2, 4, 5)),
    "interior N=3 du0 steer": (X0_INTERIOR, 3, (0, 0), (), (2, 4, 5)),
    "interior N=3 du0 accel": (X0_INTERIOR, 3, (0, 1), (), (4, 5)),
    "active N=3 du0 accel": (X0_ACTIVE, 3, (0, 1), (0, 2), (2, 4, 5)),
    "active N=3 du1 steer": (X0_ACTIVE, 3, (1, 0), (0, 2), (2, 4, 5)),
}


@pytest.mark.parametrize("case", list(CHAIN_CASES))
def test_dynamic_chain_matches_relinearised_differences(case):
    """Measured (the larger of the frozen and the total gain's deviation): interior du0 steer 1.8e-9
    (N = 2) and 6.0e-10 (N = 3), interior du0 accel 1.5e-7, active du0 accel 9.8e-8, active du1 steer
    3.0e-9, against BAR_CHAIN = 1e-5."""
    x0, N, (stage, j), active, far = CHAIN_CASES[case]
    o = run_chain(N, x0, U0, seed_of(N, stage, j), f"dyn incr {case}")
    act = o["a"].act
    on = np.flatnonzero((act == 1) | (act == 2))
    print(f"dyn incr {case}: active inequality rows {on}, du_0 {o['r0'].x[seed_of(N, 0, 0):seed_of(N, 1, 0)]}, "
          f"worst deviation {o['worst']:.1e}")
    assert np.array_equal(on, steer_rows(N)[list(active)])
    if active:
        assert np.allclose(o["r0"].x[seed_of(N, 0, 0):seed_of(N, 1, 0)], [mpc.DYN_DUMIN[0], 0.17796], rtol=1e-5)
    # the linearisation term is not small: dropping it must not pass
    gap = np.abs(o["total"] - o["frozen"])
    floor = cpu.BAR_CHAIN * np.abs(o["fd_total"]).max()
    print(f"dyn incr {case}: total - frozen {o['total'] - o['frozen']}, bar {floor:.1e}")
    assert (gap[list(far)] > 100 * floor).all()
    if case == "interior N=3 du0 steer":     # the oracle's figures of the issue this answers (yaw, vx, vy, r)
        assert np.allclose(o["frozen"][2:], [-0.49934, -4.2825e-3, -0.094241, -0.106576], rtol=2e-4)
        assert np.allclose(o["total"][2:], [-0.54903, -4.3535e-3, -0.066281, -0.071371], rtol=2e-4)
    if case == "active N=3 du0 accel":       # vy and r change sign
        assert np.allclose(o["frozen"][2:], [6.11e-4, -1.231071, -1.297e-3, -2.588e-3], rtol=2e-3)
        assert np.allclose(o["total"][2:], [-3.441e-2, -1.231142, 2.199e-2, 3.088e-2], rtol=2e-3)
