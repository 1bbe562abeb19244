"""The LTV MPC in the inputs themselves on the device (csrc/mpc_assembly.hip: mpcqp_ltv_layout,
k_ltv_assemble_vec; csrc/mpc_device.hip: k_kin_rollout, k_kin_ltv_shift; osqp_amd.mpc.ltv_qp,
osqp_amd.mpc_device.LTVLayout / rollout_kin / KinematicLTVMPC) against host restatements of
Control/MPC/mpc_kinematics_pred_matrix.py:main and the reference's own fixtures
(tests/golden/make_golden_ltv.py):

  kinltv_sim_n40.npz   three steps of main at N = 40: each step's inputs, QP, solution (the
                       oracle's, behind the osqp stub) and shifted state
  kinltv_sim_n100.npz  two steps at main's own N = 100
  kinltv_sim_n2.npz, kinltv_sim_n3.npz  three steps at the shortest horizons
  kinltv_run_n20.npz   40 steps at N = 20: plt_states / plt_actions and their sensitivity to
                       the solver tolerance (traj_sens)

and mpc.ltv_qp against the three QPs captured from mpc__, mpc and mpc_ (kin_ltv_n40.npz,
dyn_ltv_n30.npz, kin_corridor_n30.npz).  The host restatements are checked against the
fixtures on CPU, the device kernels on the GPU.

What main's tail does (the fixtures decide, not its comments): it shifts pred_x / pred_u in
place through aliases, and the result is pred_x = (x_next, S_2..S_N, update(S_N, U_{N-1})),
pred_u = (U_1..U_{N-1}, U_{N-1}, U_{N-1}): the terminal control is the solution's stage N-1.
update_kinematics_model advances v before yaw uses it.

Whole-run check (test_whole_run_within_solver_tolerance), measured on an MI355X: largest
|device - fixture| per column (x, y, v, yaw, steer, accel) over the 40 rows 1.1e-12, 2.3e-12,
2.5e-14, 1.5e-12, 4.5e-12, 5.8e-13, against traj_sens 2.0e-5, 7.9e-5, 5.4e-6, 7.4e-5, 5.5e-4,
1.1e-4.
"""
import ctypes as C
import json

import numpy as np
import pytest

from loop_checks import (EUNSUPPORTED, INF, check_assembled, check_fixture_step, check_solutions, check_whole_run, dense,
                         dev as _t, host, oracle_batch, oracle_solve, same_csc as _same_csc, sim_qp as _sim_qp,
                         stage_shift as _stage_shift)
from osqp_amd import canonical_data, mpc
from osqp_amd.mpc_device import KinVehicle, LTVLayout, _bind

L_F, L_R, DT = 1.25, 1.40, 0.02  # main's vehicle (:357-370)
W = (mpc.KINLTV_Q, mpc.KINLTV_QN, mpc.KINLTV_R)
BOUNDS = (mpc.KINLTV_XMIN, mpc.KINLTV_XMAX, mpc.KINLTV_UMIN, mpc.KINLTV_UMAX)
SETTINGS = dict(polish=False, warm_start=True)  # :347


def _layout(N, **kw):
    return LTVLayout(N, *W, *BOUNDS, mpc.KIN_MASK_A, mpc.KIN_MASK_B, **kw)


def _qp(Ad, Bd, gd, x, Xr, N):
    return mpc.ltv_qp(list(Ad), list(Bd), list(gd), x, Xr, *W, N, *BOUNDS)


# ------------------------------------------------------------------ host restatements --
def reference_search(path_x, path_y, pred_x, dt, N):
    """mpc_kinematics_pred_matrix.py:26-82 (speed 10, yaw 0): pred_x (N+1, 4) stage-major -> Xr (4, N+1)."""
    return mpc.reference_search_paths(path_x[None], path_y[None], None, None, [10.0], pred_x[None], dt)[0]


def kin_update(x, u):
    return mpc.kin_update(L_F, L_R, DT, x, u)


def rollout(x0, u0, N):
    """Initial horizon (:405-419): pred_x (N+1, 4) by the nonlinear model under u0, pred_u (N+1, 2) = u0."""
    pred_x = [np.asarray(x0, float)]
    for _ in range(N):
        pred_x.append(kin_update(pred_x[-1], u0))
    return np.stack(pred_x), np.tile(np.asarray(u0, float), (N + 1, 1))


def tail(sol, Ad0, Bd0, gd0, x, N):
    """main's loop after a `solved` solve (:486-563) without its aliasing: returns (row, x, u,
    pred_x (N+1, 4), pred_u (N+1, 2)); row = plt_states[:, i] and plt_actions[:, i]."""
    S = sol[:(N + 1) * 4].reshape(N + 1, 4)
    U = sol[(N + 1) * 4:].reshape(N, 2)
    row = np.concatenate([x, U[0]])
    x_next = Ad0 @ x + Bd0 @ U[0] + gd0
    pred_x = np.empty((N + 1, 4)); pred_u = np.empty((N + 1, 2))
    pred_x[0] = x_next
    pred_x[1:N] = S[2:N + 1]
    pred_x[N] = kin_update(S[N], U[N - 1])
    pred_u[0:N - 1] = U[1:N]
    pred_u[N - 1] = pred_u[N] = U[N - 1]
    return row, x_next, U[0].copy(), pred_x, pred_u


def loop(x0, u0, path_x, path_y, N, steps, solve):
    """main (:355-563) for one vehicle with `solve(P, q, A, l, u) -> x` always `solved`; the rows."""
    x = np.asarray(x0, float)
    pred_x, pred_u = rollout(x0, u0, N)
    rows = []
    for _ in range(steps):
        Xr = reference_search(path_x, path_y, pred_x, DT, N)
        Ad, Bd, gd = mpc.linearise_kinematics(L_F, L_R, DT, pred_x[:N], pred_u[:N])
        sol = solve(*_qp(Ad, Bd, gd, x, Xr, N))
        row, x, _, pred_x, pred_u = tail(sol, Ad[0], Bd[0], gd[0], x, N)
        rows.append(row)
    return np.stack(rows)


_oracle_solve = oracle_solve(SETTINGS)


# ----------------------------------------------------------------------- CPU tests --
@pytest.mark.parametrize("name,N", [("kinltv_sim_n2.npz", 2), ("kinltv_sim_n3.npz", 3), ("kinltv_sim_n40.npz", 40),
                                    ("kinltv_sim_n100.npz", 100)])
def test_sim_steps_restatements_match_reference(golden, name, N):
    """The captured steps of main: the host restatements reproduce each step from its inputs and
    solution, and mpc.ltv_qp reproduces each step's QP exactly."""
    g = golden(name)
    assert json.loads(str(g["settings"])) == dict(verbose=False, warm_start=True)
    px0, pu0 = rollout(g["x0"], g["u0"], N)
    assert np.allclose(px0, g["in_pred_x"][0].T, rtol=1e-12, atol=1e-12)
    assert np.array_equal(pu0, g["in_pred_u"][0].T)
    for t in range(g["in_x"].shape[0]):
        pred_x, pred_u = g["in_pred_x"][t].T, g["in_pred_u"][t].T          # (N+1, 4), (N+1, 2)
        Xr = reference_search(g["path_x"], g["path_y"], pred_x, DT, N)
        assert np.array_equal(Xr, g["in_Xr"][t])
        assert (Xr[2] == 10.0).all() and (Xr[3] == 0.0).all()
        Ad, Bd, gd = mpc.linearise_kinematics(L_F, L_R, DT, pred_x[:N], pred_u[:N])
        assert np.allclose(Ad, g["in_Ad"][t], rtol=1e-13, atol=1e-15)
        assert np.allclose(Bd, g["in_Bd"][t], rtol=1e-13, atol=1e-15)
        assert np.allclose(gd, g["in_gd"][t], rtol=1e-13, atol=1e-15)
        P, q, A, l, u = _qp(g["in_Ad"][t], g["in_Bd"][t], g["in_gd"][t], g["in_x"][t], g["in_Xr"][t], N)
        Pr, qr, Ar, lr, ur = _sim_qp(g, t)
        assert _same_csc(P, Pr) and _same_csc(A, Ar)
        assert np.array_equal(dense(P), dense(Pr)) and np.array_equal(dense(A), dense(Ar))
        assert np.array_equal(q, qr) and np.array_equal(l, lr) and np.array_equal(u, ur)
        row, x, uu, px, pu = tail(g["sol"][t], g["in_Ad"][t][0], g["in_Bd"][t][0], g["in_gd"][t][0], g["in_x"][t], N)
        assert np.allclose(x, g["out_x"][t], rtol=1e-12, atol=1e-12)
        assert np.allclose(px, g["out_pred_x"][t].T, rtol=1e-12, atol=1e-12)
        assert np.array_equal(pu, g["out_pred_u"][t].T)                    # copies: bit for bit
        assert np.array_equal(px[1:N], g["out_pred_x"][t].T[1:N])
        assert np.array_equal(row, g["out_row"][t])
    # consecutive steps chain: a step's output is the next step's input
    assert np.array_equal(g["out_x"][:-1], g["in_x"][1:]) and np.array_equal(g["out_pred_x"][:-1], g["in_pred_x"][1:])
    assert np.array_equal(g["out_pred_u"][:-1], g["in_pred_u"][1:])


def test_whole_loop_restatement_matches_reference(golden):
    g = golden("kinltv_run_n20.npz")
    rows = loop(g["x0"], g["u0"], g["path_x"], g["path_y"], int(g["N"]), int(g["steps"]), _oracle_solve)
    assert rows.shape == g["traj"].shape == (40, 6)
    assert np.allclose(rows, g["traj"], rtol=1e-12, atol=1e-12)
    assert (g["traj_sens"] > 0).all()


def _kin_rollout_lin(x0, u0, N):
    """The generators' linearised rollout (make_golden.py:_kin_rollout)."""
    Ads, Bds, gds = [], [], []
    xk = x0.copy()
    for _ in range(N):
        A_, B_, g_ = (v[0] for v in mpc.linearise_kinematics(L_F, L_R, DT, xk, u0))
        Ads.append(A_); Bds.append(B_); gds.append(g_)
        xk = A_ @ xk + B_ @ u0 + g_
    return Ads, Bds, gds


def _check_qp(got, g):
    P, q, A, l, u = got
    assert _same_csc(P, g["P"]) and _same_csc(A, g["A"])
    assert np.array_equal(dense(P), dense(g["P"]))
    assert np.array_equal(q, g["q"]) and np.array_equal(l[A.shape[1]:], g["l"][A.shape[1]:])
    assert np.array_equal(u[A.shape[1]:], g["u"][A.shape[1]:])
    assert np.allclose(dense(A), dense(g["A"]), rtol=1e-12, atol=1e-12)
    neq = A.shape[0] - A.shape[1]
    assert np.allclose(l[:neq], g["l"][:neq], rtol=1e-12, atol=1e-12)
    assert np.allclose(u[:neq], g["u"][:neq], rtol=1e-12, atol=1e-12)


def test_ltv_qp_reproduces_mpc__(golden):
    """kin_ltv_n40.npz (mpc_kinematics_pred_matrix.mpc__); inputs rebuilt from make_golden.kin_ltv's constants."""
    N = 40
    x0 = np.array([0.0, 0.5, 20.0, np.deg2rad(3.0)]); u0 = np.array([np.deg2rad(1.0), 0.01])
    Ads, Bds, gds = _kin_rollout_lin(x0, u0, N)
    Xr = np.zeros((4, N + 1)); Xr[0] = np.arange(N + 1) * 20.0 * 0.02; Xr[2] = 20.0
    _check_qp(mpc.ltv_qp(Ads, Bds, gds, x0, Xr, *W, N, *BOUNDS), golden("kin_ltv_n40.npz"))


def test_ltv_qp_reproduces_dynamic_mpc(golden):
    """dyn_ltv_n30.npz (mpc_dynamics.mpc, nx 6); inputs rebuilt from make_golden.dyn_ltv's constants."""
    N = 30
    veh = mpc.VehicleParams(dt=0.05)
    x0 = np.array([0., 0.5, np.deg2rad(4.0), 12.0, 0.1, 0.02]); u0 = np.array([np.deg2rad(1.0), 0.2])
    Ads, Bds, gds = [], [], []
    xk = x0.copy()
    for _ in range(N):
        A_, B_, g_ = (v[0] for v in mpc.linearise_dynamics(veh, xk[None], u0[None]))
        Ads.append(A_); Bds.append(B_); gds.append(g_)
        xk = A_ @ xk + B_ @ u0 + g_
    # the masks are the structural nonzeros of this model
    assert not np.stack(Ads)[:, mpc.DYN_MASK_A == 0].any() and not np.stack(Bds)[:, mpc.DYN_MASK_B == 0].any()
    Xr = np.zeros((6, N + 1)); Xr[0] = np.arange(N + 1) * 10.0 * 0.05; Xr[3] = 10.0
    xmin = np.array([-np.inf, -np.inf, -2 * np.pi, -100., -30., -0.5 * np.pi])
    _check_qp(mpc.ltv_qp(Ads, Bds, gds, x0, Xr, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, N, xmin, -xmin,
                         mpc.KINLTV_UMIN, mpc.KINLTV_UMAX), golden("dyn_ltv_n30.npz"))


def test_ltv_qp_reproduces_corridor(golden):
    """kin_corridor_n30.npz (mpc_kinematics.mpc_): one model on every stage, per-stage state
    bounds read back from the fixture's own l / u."""
    g = golden("kin_corridor_n30.npz")
    N = 30
    x0 = np.array([0.0, 0.3, 10.0, np.deg2rad(2.0)]); u0 = np.array([0.0, 0.0])
    Ad, Bd, gd = (v[0] for v in mpc.linearise_kinematics(L_F, L_R, DT, x0, u0))
    Xr = np.zeros((4, N + 1)); Xr[0] = np.arange(N + 1) * 10.0 * 0.02; Xr[2] = 10.0
    ns = (N + 1) * 4
    xlo, xhi = g["l"][ns:2 * ns].reshape(N + 1, 4), g["u"][ns:2 * ns].reshape(N + 1, 4)
    assert (np.diff(xlo[:, 0]) > 0).all() and (xlo[:, 2] == -10).all() and (xhi[:, 3] == np.pi).all()
    _check_qp(mpc.ltv_qp([Ad] * N, [Bd] * N, [gd] * N, x0, Xr, mpc.KINLTV_Q, mpc.KINLTV_Q, mpc.KINLTV_R, N,
                         None, None, mpc.KINLTV_UMIN, mpc.KINLTV_UMAX, xlo=xlo, xhi=xhi), g)


def _dyn_layout(N):
    xmin = np.array([-np.inf, -np.inf, -2 * np.pi, -100., -30., -0.5 * np.pi])
    return (LTVLayout(N, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, xmin, -xmin, mpc.KINLTV_UMIN, mpc.KINLTV_UMAX,
                      mpc.DYN_MASK_A, mpc.DYN_MASK_B),
            lambda Ad, Bd, gd, x0, Xr: mpc.ltv_qp(Ad, Bd, gd, x0, Xr, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, N, xmin, -xmin,
                                                  mpc.KINLTV_UMIN, mpc.KINLTV_UMAX), mpc.DYN_MASK_A, mpc.DYN_MASK_B)


def _kin_layout(N):
    return (_layout(N), lambda Ad, Bd, gd, x0, Xr: _qp(Ad, Bd, gd, x0, Xr, N), mpc.KIN_MASK_A, mpc.KIN_MASK_B)


@pytest.mark.parametrize("N", [2, 3, 40])
@pytest.mark.parametrize("make", [_kin_layout, _dyn_layout], ids=["nx4", "nx6"])
def test_layout_pattern_matches_host_builder(make, N):
    L, build, mA, mB = make(N)
    nx, nu = mA.shape[0], mB.shape[1]
    P, A, lt, ut = L.pattern()
    assert (L.n, L.m) == ((N + 1) * nx + N * nu, 2 * (N + 1) * nx + N * nu)
    assert (L.nnzP, L.nnzA) == (P.nnz, A.nnz)
    P2, _, A2, l2, u2 = build([np.where(mA, 7.0, 0.0)] * N, [np.where(mB, 7.0, 0.0)] * N, [np.zeros(nx)] * N,
                              np.zeros(nx), np.zeros((nx, N + 1)))
    P2, A2 = canonical_data(P2, A2)
    assert np.array_equal(P.indptr, P2.indptr) and np.array_equal(P.indices, P2.indices)
    assert np.array_equal(P.data, P2.data)
    assert np.array_equal(A.indptr, A2.indptr) and np.array_equal(A.indices, A2.indices)
    const = A2.data != 7.0
    assert np.array_equal(A.data[const], A2.data[const]) and not A.data[~const].any()
    box = slice((N + 1) * nx, None)
    assert np.array_equal(lt[box], np.clip(l2[box], -INF, INF)) and np.array_equal(ut[box], np.clip(u2[box], -INF, INF))
    assert not lt[:(N + 1) * nx].any() and not ut[:(N + 1) * nx].any()


def _raw_kin_ltv_shift(L, B, sol, status, Ad, Bd, gd, x, u, px, pu, skipped, steps, traj, cap, tlen, ptr):
    return _bind().mpcqp_kin_ltv_shift_device(L._h, C.byref(KinVehicle()), B, ptr(sol), None if status is None else
                                              ptr(status), ptr(Ad), ptr(Bd), ptr(gd), ptr(x), ptr(u), ptr(px),
                                              ptr(pu), ptr(skipped), ptr(steps), ptr(traj), cap, ptr(tlen), None)


def test_argument_errors_are_unsupported():
    from osqp_amd import lib
    with pytest.raises(NotImplementedError):       # MPCQP_EUNSUPPORTED
        LTVLayout(4, np.eye(7), np.eye(7), np.eye(2), -np.ones(7), np.ones(7), -np.ones(2), np.ones(2),
                  np.eye(7, dtype=np.uint8), np.ones((7, 2), np.uint8))
    with pytest.raises(NotImplementedError):
        LTVLayout(4, np.eye(4), np.eye(4), np.eye(3), -np.ones(4), np.ones(4), -np.ones(3), np.ones(3),
                  np.eye(4, dtype=np.uint8), np.ones((4, 3), np.uint8))
    with pytest.raises(NotImplementedError):
        _layout(1)
    # the kinematic shift handed an nx-6 layout: refused before anything is read or launched
    # (the buffers are host arrays that only have to be non-NULL)
    L6 = _dyn_layout(4)[0]
    z = np.zeros(8)
    zi = np.zeros(2, np.int32)
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    assert _raw_kin_ltv_shift(L6, 1, z, None, z, z, z, z, z, z, z, zi, zi, z, 0, zi, ptr) == EUNSUPPORTED
    assert b"nx 4" in lib().mpcqp_last_error()
    assert not z.any() and not zi.any()


# ------------------------------------------------------------------------- GPU tests --
def _rep(a, B):
    """B instances cycling through the leading axis of a."""
    return np.ascontiguousarray(a[np.arange(B) % a.shape[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("name,N,B", [("kinltv_sim_n40.npz", 40, 3), ("kinltv_sim_n40.npz", 40, 130),
                                      ("kinltv_sim_n100.npz", 100, 2)])
def test_assembly_matches_reference_qps(golden, name, N, B):
    """mpcqp_ltv_assemble_device on the captured steps' inputs against the reference's own QPs
    (B = 130: a full 128-thread block of the vector kernel plus a partial one)."""
    g = golden(name)
    T = g["in_x"].shape[0]
    L = _layout(N)
    args = [_t(_rep(g[k], B)) for k in ("in_Ad", "in_Bd", "in_gd", "in_x", "in_Xr")]
    Ax, q, l, u = (v.cpu().numpy() for v in L.assemble(*args))
    Apat = L.pattern()[1]
    for b in range(B):
        Pr, qr, Ar, lr, ur = _sim_qp(g, b % T)
        if b < T or b >= B - T:
            A_dev = Apat.copy(); A_dev.data = Ax[b]
            assert np.allclose(dense(A_dev), dense(Ar), rtol=1e-15, atol=0)
        else:
            assert np.array_equal(Ax[b], Ax[b % T])
        assert np.allclose(q[b], qr, rtol=1e-15, atol=0)
        assert np.array_equal(l[b], np.clip(lr, -INF, INF)) and np.array_equal(u[b], np.clip(ur, -INF, INF))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 130])
def test_assembly_with_corridor_bounds(golden, B):
    """Per-instance, per-stage state bounds (xlo / xhi, incl. +-inf) replace the state rows of the
    box and nothing else; with one of them NULL that side keeps the layout's bounds."""
    g = golden("kinltv_sim_n40.npz")
    N, ns = 40, 41 * 4
    L = _layout(N)
    args = [_t(_rep(g[k], B)) for k in ("in_Ad", "in_Bd", "in_gd", "in_x", "in_Xr")]
    rng = np.random.default_rng(5)
    xlo = -rng.uniform(0.5, 3.0, (B, N + 1, 4)); xhi = rng.uniform(0.5, 3.0, (B, N + 1, 4))
    xlo[:, :, 3] = -np.inf; xhi[:, ::2, 2] = np.inf; xlo[-1, -1, 0] = -2e30
    base = [v.cpu().numpy() for v in L.assemble(*args)]
    both = [v.cpu().numpy() for v in L.assemble(*args, xlo=_t(xlo), xhi=_t(xhi))]
    lo_only = [v.cpu().numpy() for v in L.assemble(*args, xlo=_t(xlo))]
    for got, lo, hi in ((both, xlo, xhi), (lo_only, xlo, None)):
        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1])
        l_want, u_want = base[2].copy(), base[3].copy()
        l_want[:, ns:2 * ns] = np.clip(lo.reshape(B, ns), -INF, INF)
        if hi is not None:
            u_want[:, ns:2 * ns] = np.clip(hi.reshape(B, ns), -INF, INF)
        assert np.array_equal(got[2], l_want) and np.array_equal(got[3], u_want)
    # and the host builder says the same for one instance
    b = B - 1
    _, _, _, l2, u2 = mpc.ltv_qp(list(g["in_Ad"][b % 3]), list(g["in_Bd"][b % 3]), list(g["in_gd"][b % 3]),
                                 g["in_x"][b % 3], g["in_Xr"][b % 3], *W, N, *BOUNDS, xlo=xlo[b], xhi=xhi[b])
    assert np.array_equal(both[2][b], np.clip(l2, -INF, INF)) and np.array_equal(both[3][b], np.clip(u2, -INF, INF))


def _shift(L, sol, status, Ad, Bd, gd, x, u, px, pu, skipped, steps, traj, cap, tlen):
    """mpcqp_kin_ltv_shift_device on device tensors, on the null stream; returns the call's code."""
    import torch
    from osqp_amd.mpc_device import _p
    code = _raw_kin_ltv_shift(L, x.shape[0], sol, status, Ad, Bd, gd, x, u, px, pu, skipped, steps, traj, cap, tlen,
                              _p)
    torch.cuda.synchronize()
    return code


def _host_case(N, B, seed):
    """B seeded (state, horizon model, solution) cases at horizon N with the host tail's results."""
    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(-5, 5, B), rng.uniform(-5, 5, B), rng.uniform(2, 25, B), rng.uniform(-1, 1, B)], 1)
    u = np.stack([np.deg2rad(rng.uniform(-10, 10, B)), rng.uniform(-2, 1, B)], 1)
    Ad, Bd, gd = mpc.linearise_kinematics(L_F, L_R, DT, x, u)
    Ad, Bd, gd = (np.ascontiguousarray(np.repeat(v[:, None], N, 1)) for v in (Ad, Bd, gd))
    sol = rng.uniform(-1, 1, (B, (N + 1) * 4 + N * 2))
    sol[:, 2:(N + 1) * 4:4] += 10.0
    want = [tail(sol[b], Ad[b, 0], Bd[b, 0], gd[b, 0], x[b], N) for b in range(B)]
    return x, u, Ad, Bd, gd, sol, [np.stack([w[i] for w in want]) for i in range(5)]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 130])
@pytest.mark.parametrize("N", [2, 3, 40])
def test_rollout_and_shift_match_host(golden, N, B):
    """k_kin_rollout and k_kin_ltv_shift against the fixture's own post-shift state (the captured
    steps of main take the first places of the batch) and, for the seeded rest of the batch,
    against the host restatements (which the CPU tests hold to the fixtures)."""
    import torch
    from osqp_amd.mpc_device import rollout_kin
    x, u, Ad, Bd, gd, sol, (rows, xn, un, pxn, pun) = _host_case(N, B, 100 * N + B)
    g = golden(f"kinltv_sim_n{N}.npz")
    T = min(B, 3)
    x[:T], sol[:T] = g["in_x"][:T], g["sol"][:T]
    Ad[:T], Bd[:T], gd[:T] = g["in_Ad"][:T], g["in_Bd"][:T], g["in_gd"][:T]
    xn[:T], pxn[:T], pun[:T] = g["out_x"][:T], g["out_pred_x"][:T].transpose(0, 2, 1), \
        g["out_pred_u"][:T].transpose(0, 2, 1)
    rows[:T], un[:T] = g["out_row"][:T], g["out_row"][:T, 4:]
    veh, L = KinVehicle(), _layout(N)
    px, pu = rollout_kin(veh, _t(x), _t(u), N)
    for b in range(B):
        wx, wu = rollout(x[b], u[b], N)
        assert np.allclose(px[b].cpu().numpy(), wx, rtol=1e-12, atol=1e-12) and np.array_equal(pu[b].cpu().numpy(), wu)
    xd, ud = _t(x), _t(u)
    skipped, steps, tlen = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    traj = torch.zeros((B, 2, 6), dtype=torch.float64, device="cuda")
    assert _shift(L, _t(sol), None, _t(Ad), _t(Bd), _t(gd), xd, ud, px, pu, skipped, steps, traj, 2, tlen) == 0
    assert np.allclose(xd.cpu().numpy(), xn, rtol=1e-12, atol=1e-12)
    assert np.array_equal(ud.cpu().numpy(), un)
    assert np.allclose(px.cpu().numpy(), pxn, rtol=1e-12, atol=1e-12)
    assert np.array_equal(px[:, 1:N].cpu().numpy(), pxn[:, 1:N])           # copies: bit for bit
    assert np.array_equal(pu.cpu().numpy(), pun)
    assert np.array_equal(traj[:, 0].cpu().numpy(), rows) and not traj[:, 1].any()
    assert (tlen == 1).all() and (steps == 1).all() and not skipped.any()


@pytest.mark.gpu
def test_skip_rule_at_the_entry_point():
    """A crafted status vector: every vehicle whose status is not 1 (solved inaccurate 2, max
    iterations -2, an unknown 7) keeps all its state bit for bit and counts one skip; the
    others equal an all-solved call."""
    import torch
    N, B = 5, 130
    x, u, Ad, Bd, gd, sol, _ = _host_case(N, B, 9)
    status = np.array([1, 2, -2, 7, 1, 1, -2], np.int32)[np.arange(B) % 7]
    ok = status == 1
    L = _layout(N)
    rng = np.random.default_rng(3)
    px0, pu0 = rng.normal(size=(B, N + 1, 4)), rng.normal(size=(B, N + 1, 2))
    traj0 = rng.normal(size=(B, 3, 6))

    def run(st):
        s = dict(x=_t(x), u=_t(u), px=_t(px0), pu=_t(pu0), traj=_t(traj0),
                 skipped=torch.zeros(B, dtype=torch.int32, device="cuda"),
                 steps=torch.full((B,), 4, dtype=torch.int32, device="cuda"),
                 tlen=torch.ones(B, dtype=torch.int32, device="cuda"))
        assert _shift(L, _t(sol), None if st is None else _t(st, torch.int32), _t(Ad), _t(Bd), _t(gd), s["x"], s["u"],
                      s["px"], s["pu"], s["skipped"], s["steps"], s["traj"], 3, s["tlen"]) == 0
        return {k: v.cpu().numpy() for k, v in s.items()}

    got, ref = run(status), run(None)
    for k, before in (("x", x), ("u", u), ("px", px0), ("pu", pu0), ("traj", traj0)):
        assert np.array_equal(got[k][~ok], before[~ok]), k
        assert np.array_equal(got[k][ok], ref[k][ok]), k
        assert not np.array_equal(ref[k][~ok], before[~ok]), k
    assert np.array_equal(got["skipped"], (~ok).astype(np.int32)) and not ref["skipped"].any()
    assert np.array_equal(got["steps"], 4 + ok) and (ref["steps"] == 5).all()
    assert np.array_equal(got["tlen"], 1 + ok) and (ref["tlen"] == 2).all()


def _starts(B):
    """Distinct starts beside main's path (y = -5)."""
    x0 = np.zeros((B, 4))
    x0[:, 0] = np.linspace(0.0, 40.0, B)
    x0[:, 1] = -5.0 + np.array([5.0, 1.0, -2.0, 3.5, -4.0, 2.0])[np.arange(B) % 6]
    x0[:, 2] = np.array([20.0, 12.0, 8.0, 15.0, 10.0, 18.0])[np.arange(B) % 6]
    x0[:, 3] = np.deg2rad([0.0, 4.0, -3.0, -6.0, 8.0, 1.0])[np.arange(B) % 6]
    u0 = np.tile([0.0, 0.01], (B, 1)); u0[1::2, 0] = np.deg2rad(1.0)
    return x0, u0


def _main_path():
    px = np.linspace(-10, 100, 200)
    return px, px * 0.0 - 5.0


def _check_step(ctl, before, N, status, Ppat, Apat, Px):
    """One step of the class against the host restatement fed the device's own state, the oracle
    on that QP, and the host tail of the device's own solution."""
    x, pred_x, pred_u = before
    px, py = _main_path()
    B = x.shape[0]
    last, sol = host(ctl)
    for b in range(B):
        Xr = reference_search(px, py, pred_x[b], DT, N)
        assert np.array_equal(last["Xr"][b], Xr)
        Ad, Bd, gd = mpc.linearise_kinematics(L_F, L_R, DT, pred_x[b, :N], pred_u[b, :N])
        check_assembled(last, b, Ad, Bd, gd, _qp(Ad, Bd, gd, x[b], Xr, N), Apat)
    ro = oracle_batch(last, status, Ppat, Apat, Px, SETTINGS)
    check_solutions(sol, ro.x, slice((N + 1) * 4, None))
    for b in range(B):
        row, xn, un, pxn, pun = tail(sol[b], last["Ad"][b, 0], last["Bd"][b, 0], last["gd"][b, 0], x[b], N)
        assert np.allclose(ctl.x[b].cpu().numpy(), xn, rtol=1e-13, atol=1e-13)
        assert np.array_equal(ctl.u[b].cpu().numpy(), un)
        assert np.allclose(ctl.pred_x[b].cpu().numpy(), pxn, rtol=1e-10, atol=1e-10)
        assert np.array_equal(ctl.pred_u[b].cpu().numpy(), pun)
    return ro


def _state(ctl):
    return tuple(v.cpu().numpy() for v in (ctl.x, ctl.pred_x, ctl.pred_u))


@pytest.mark.gpu
@pytest.mark.parametrize("N,variant", [(10, 4), (40, 11)])
def test_closed_loop_matches_host_restatement(N, variant):
    from osqp_amd.mpc_device import KinematicLTVMPC
    B, steps = 6, 4
    x0, u0 = _starts(B)
    px, py = _main_path()
    ctl = KinematicLTVMPC(x0, u0, px, py, N=N, traj_cap=3)
    assert ctl.solver.plan_info()["variant"] == variant
    for b in range(B):
        wx, wu = rollout(x0[b], u0[b], N)
        assert np.allclose(ctl.pred_x[b].cpu().numpy(), wx, rtol=1e-12, atol=1e-12)
        assert np.array_equal(ctl.pred_u[b].cpu().numpy(), wu)
    P, Apat, _, _ = ctl.layout.pattern()
    Px = np.tile(P.data, (B, 1))
    rows = []
    n_iter_match = 0
    for _ in range(steps):
        before = _state(ctl)
        status, iters = ctl.step()
        ro = _check_step(ctl, before, N, status.cpu().numpy(), P, Apat, Px)
        n_iter_match += int((iters.cpu().numpy() == ro.iter).sum())
        rows.append(np.concatenate([before[0], ctl.u.cpu().numpy()], 1))
    assert n_iter_match >= 0.9 * B * steps
    assert (ctl.steps_taken.cpu().numpy() == steps).all() and not ctl.skipped.any()
    # trajectory cap: rows beyond traj_cap are dropped
    traj, tlen = ctl.trajectories()
    assert traj.shape == (B, 3, 6) and np.array_equal(tlen, np.full(B, 3))
    assert np.array_equal(traj, np.stack(rows[:3], 1))


@pytest.mark.gpu
def test_one_step_at_the_shipped_horizon(golden):
    """N = 100 (main's own), B = 2: vehicle 0 is the fixture's first step, vehicle 1 its second
    (state and horizon set from the fixture)."""
    from osqp_amd.mpc_device import KinematicLTVMPC
    g = golden("kinltv_sim_n100.npz")
    N = 100
    ctl = KinematicLTVMPC(np.tile(g["x0"], (2, 1)), np.tile(g["u0"], (2, 1)), g["path_x"], g["path_y"])
    assert ctl.N == N
    info = ctl.solver.plan_info()
    print("plan_info N=100:", info)
    assert info["lds_bytes_solve"] <= 160 * 1024 and info["variant"] in (11, 12, 13) and info["threads_per_qp"] == 512
    assert np.allclose(ctl.pred_x[0].cpu().numpy(), g["in_pred_x"][0].T, rtol=1e-12, atol=1e-12)
    ctl.x[1] = _t(g["in_x"][1]); ctl.pred_x[1] = _t(g["in_pred_x"][1].T); ctl.pred_u[1] = _t(g["in_pred_u"][1].T)
    P, Apat, _, _ = ctl.layout.pattern()
    before = _state(ctl)
    status, iters = ctl.step()
    _check_step(ctl, before, N, status.cpu().numpy(), P, Apat, np.tile(P.data, (2, 1)))
    check_fixture_step(ctl, g, Apat, slice((N + 1) * 4, None))
    print("iters", iters.cpu().numpy(), "fixture", g["sol_iter"])


@pytest.mark.gpu
def test_skip_rule_at_the_class():
    """max_iter = 10: no solve ends `solved`, so nothing moves and every step counts as skipped."""
    from osqp_amd.mpc_device import KinematicLTVMPC
    x0, u0 = _starts(3)
    px, py = _main_path()
    ctl = KinematicLTVMPC(x0, u0, px, py, N=10, traj_cap=4, max_iter=10)
    before = _state(ctl)
    for _ in range(3):
        status, _ = ctl.step()
        assert (status.cpu().numpy() != 1).all()
    after = _state(ctl)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.array_equal(ctl.x.cpu().numpy(), x0) and np.array_equal(ctl.u.cpu().numpy(), u0)
    assert (ctl.steps_taken.cpu().numpy() == 0).all() and (ctl.skipped.cpu().numpy() == 3).all()
    traj, tlen = ctl.trajectories()
    assert not traj.any() and not tlen.any()


@pytest.mark.gpu
def test_whole_run_within_solver_tolerance(golden):
    """The 40-step run of kinltv_run_n20.npz on the device: rounding inside ADMM must move the
    trajectory less than the solver tolerance does (traj_sens: the same run of the reference
    with the oracle at eps 1e-6 against eps 1e-3).  Two copies of the vehicle stay identical."""
    from osqp_amd.mpc_device import KinematicLTVMPC
    g = golden("kinltv_run_n20.npz")
    steps = int(g["steps"])
    ctl = KinematicLTVMPC(np.tile(g["x0"], (2, 1)), np.tile(g["u0"], (2, 1)), g["path_x"], g["path_y"], N=int(g["N"]),
                          traj_cap=steps + 2)
    status, _ = ctl.run(steps)
    traj, tlen = ctl.trajectories()
    assert np.array_equal(tlen, [steps, steps]) and not ctl.skipped.any() and (status.cpu().numpy() == 1).all()
    check_whole_run(traj, steps, g)


@pytest.mark.gpu
def test_shift_warm_matches_oracle():
    """shift_warm=True (an extension): every step's solve starts from the previous solution
    shifted one stage; the oracle, warm-started from the same shifted iterates on the step's
    QP, ends with the same statuses (and the same controls where the iterations agree)."""
    import pyoracle
    from osqp_amd.mpc_device import KinematicLTVMPC
    B, N, steps = 12, 10, 4
    x0, u0 = _starts(B)
    px, py = _main_path()
    cold = KinematicLTVMPC(x0, u0, px, py, N=N)
    warm = KinematicLTVMPC(x0, u0, px, py, N=N, shift_warm=True)
    P, A, _, _ = warm.layout.pattern()
    Px = np.tile(P.data, (B, 1))
    du = slice((N + 1) * 4, None)
    ic = iw = match = 0
    prev = None
    for _ in range(steps):
        _, itc = cold.step()
        sw, itw = warm.step()
        ic += int(itc.sum()); iw += int(itw.sum())
        last = {k: v.cpu().numpy() for k, v in warm.last.items()}
        ws = {} if prev is None else dict(x0=_stage_shift(prev[0], N, 4, 2, 1), y0=_stage_shift(prev[1], N, 4, 2, 2))
        ro = pyoracle.solve_batch(P, A, Px, last["q"], last["Ax"], last["l"], last["u"], nthreads=8, **SETTINGS, **ws)
        assert np.array_equal(sw.cpu().numpy(), ro.status_val)
        x = warm.sol.cpu().numpy()
        same = ro.iter == itw.cpu().numpy()
        match += int(same.sum())
        assert np.abs(x[same][:, du] - ro.x[same][:, du]).max() < 1e-4
        prev = (x, warm.y.cpu().numpy())
    assert match >= 0.9 * B * steps
    assert iw < ic
