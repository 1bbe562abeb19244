"""What the device-loop test modules (test_{mpc,kin,ltv,lat,lane,kinfrozen}_device.py) share: the
fixtures' QPs, the oracle behind a `solve` callable, and the comparisons every closed loop is held
to -- the assembled step against the host builder, the solutions against the oracle's, one step
against the fixture's QP, the whole run against the solver tolerance's own effect.  A plain module,
imported like parity.py; each loop's state, tail and paths stay in its own module."""
import numpy as np
import scipy.sparse as sparse

INF = 1e30  # OSQP_INFTY: bounds are clipped to it (osqp 0.6 osqp_setup / update_bounds)
EINVAL, EUNSUPPORTED = 1, 2  # MPCQP_EINVAL, MPCQP_EUNSUPPORTED (include/mpcqp.h)


def dense(M):
    return np.asarray(M.todense())


def same_csc(M, Mr):
    """The same pattern once explicit zeros are gone (scipy's kron / block_diag of the
    reference's DIA weights store some; the host builders drop them)."""
    M, Mr = sparse.csc_matrix(M, copy=True), sparse.csc_matrix(Mr, copy=True)
    M.eliminate_zeros(); Mr.eliminate_zeros()
    M.sort_indices(); Mr.sort_indices()
    return np.array_equal(M.indptr, Mr.indptr) and np.array_equal(M.indices, Mr.indices)


def sim_qp(g, t):
    """(P, q, A, l, u) of captured step t of a *_sim_* / *_main_* fixture."""
    A = sparse.csc_matrix((g[f"A{t}_data"], g[f"A{t}_indices"], g[f"A{t}_indptr"]), shape=tuple(g[f"A{t}_shape"]))
    return g["P"], g["q"][t], A, g["l"][t], g["u"][t]


def oracle_solve(settings):
    """solve(P, q, A, l, u) -> x by a fresh oracle object with `settings`; the solve must end `solved`."""
    def solve(P, q, A, l, u):
        import pyoracle
        o = pyoracle.OSQP()
        o.setup(P, q, A, l, u, **settings)
        r = o.solve()
        assert r.info.status == "solved"
        return r.x
    return solve


def dev(a, dtype=None):
    """a as a contiguous device tensor (float64 unless dtype says otherwise)."""
    import torch
    return torch.tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device="cuda")


def stage_shift(v, N, nxa, nu, groups):
    """One-stage shift of a layout's iterates (mpcqp_incr_warm_shift_device; the reference's horizon
    shift, mpc_dynamics.py:589-610): `groups` blocks of N+1 stages of nxa, then N stages of nu; the
    last stage of each is repeated."""
    B = v.shape[0]
    out = []
    for g in range(groups):
        blk = v[:, g * (N + 1) * nxa:(g + 1) * (N + 1) * nxa].reshape(B, N + 1, nxa)
        out.append(np.concatenate([blk[:, 1:], blk[:, -1:]], 1).reshape(B, -1))
    d = v[:, groups * (N + 1) * nxa:].reshape(B, N, nu)
    out.append(np.concatenate([d[:, 1:], d[:, -1:]], 1).reshape(B, -1))
    return np.concatenate(out, 1)


def host(ctl):
    """(ctl.last as host arrays, ctl.sol as a host array)."""
    return {k: v.cpu().numpy() for k, v in ctl.last.items()}, ctl.sol.cpu().numpy()


def check_assembled(last, b, Ad, Bd, gd, qp, Apat):
    """Vehicle b's step as the device assembled it (`last`: the class's record of the step, host
    arrays) against the host linearisation Ad, Bd, gd and the host builder's qp = (P, q, A, l, u)."""
    _, q, A, l, u = qp
    assert np.allclose(last["Ad"][b], Ad, rtol=1e-13, atol=1e-15)
    assert np.allclose(last["Bd"][b], Bd, rtol=1e-13, atol=1e-15)
    assert np.allclose(last["gd"][b], gd, rtol=1e-12, atol=1e-13)
    A_dev = Apat.copy(); A_dev.data = last["Ax"][b]
    assert np.allclose(dense(A_dev), dense(A), rtol=1e-12, atol=1e-15)
    assert np.allclose(last["q"][b], q, rtol=1e-12, atol=1e-12)
    assert np.allclose(last["l"][b], np.clip(l, -INF, INF), rtol=1e-12, atol=1e-14)
    assert np.allclose(last["u"][b], np.clip(u, -INF, INF), rtol=1e-12, atol=1e-14)


def oracle_batch(last, status, Ppat, Apat, Px, settings, warm=None):
    """The oracle on the QPs the device assembled, optionally warm-started (warm: x0=, y0=); the
    device's statuses must be the oracle's, all `solved`."""
    import pyoracle
    ro = pyoracle.solve_batch(Ppat, Apat, Px, last["q"], last["Ax"], last["l"], last["u"], nthreads=8, **settings,
                              **(warm or {}))
    assert np.array_equal(status, ro.status_val) and (status == 1).all()
    return ro


def check_solutions(sol, ref, du):
    """Device solutions sol (B, n) against ref (B, n): the whole primal vector to 1e-5 of its
    scale, the controls (the slice du) to 1e-4."""
    for b in range(len(sol)):
        scale = max(1.0, np.abs(ref[b]).max())
        assert np.abs(sol[b] - ref[b]).max() < 1e-5 * scale, b
        assert np.abs(sol[b, du] - ref[b, du]).max() < 1e-4, b


def check_fixture_step(ctl, g, Apat, du):
    """test_one_step_at_the_shipped_horizon: vehicle b's assembled QP and solution against captured
    step b of the fixture g, for its first two steps."""
    last, sol = host(ctl)
    for b in range(2):
        _, qr, Ar, lr, ur = sim_qp(g, b)
        A_dev = Apat.copy(); A_dev.data = last["Ax"][b]
        assert np.allclose(dense(A_dev), dense(Ar), rtol=1e-12, atol=1e-15)
        assert np.allclose(last["q"][b], qr, rtol=1e-12, atol=1e-12)
        assert np.allclose(last["l"][b], np.clip(lr, -INF, INF), rtol=1e-12, atol=1e-14)
    check_solutions(sol[:2], g["sol"][:2], du)


def check_whole_run(traj, steps, g):
    """test_whole_run_within_solver_tolerance: two copies of the vehicle stay identical, nothing is
    recorded past `steps`, and every column stays within traj_sens of the fixture's trajectory."""
    assert np.array_equal(traj[0], traj[1]) and not traj[:, steps:].any()
    err = np.abs(traj[0, :steps] - g["traj"]).max(0)
    print("max |device - fixture| per column", err, "traj_sens", g["traj_sens"])
    assert (err < g["traj_sens"]).all(), (err, g["traj_sens"])
