"""Kinematic-bicycle closed loop on the device (csrc/mpc_linearise.hip: k_kin_linearise;
csrc/mpc_device.hip: k_kin_reference, k_kin_shift; osqp_amd.mpc_device.KinematicMPC) against host restatements
of Control/MPC/mpc_incre_kine_func.py:simulate and the reference's own fixtures
(tests/golden/make_golden_kin.py):

  kin_linearise.npz  Vehicle_Kinematics.get_kinematics_model at 48 seeded (x, u)
  kin_refsearch.npz  reference_search / nearest_point (:28-81) on main()'s path, non-zero path_yaw
  kin_sim_n40.npz    three steps of simulate: each step's inputs, QP, solution (the oracle's,
                     behind the osqp stub) and shifted state
  kin_stop_n40.npz   the whole run until simulate's stop rule breaks the loop: the trajectory
                     lists, the step count, the stop-rule distances and the trajectories'
                     sensitivity to the solver tolerance (traj_sens)

The host restatements are checked against the fixtures on CPU, the device kernels on the GPU.

What the reference's shift does (the fixtures decide, not its comments): simulate shifts
pred_x~ IN PLACE (temp_pred_x_tilda is pred_x_tilda), so the control of the terminal Euler
step, read from column N-1 after that column was overwritten with column N, is the
solution's stage-N control; update_kinematics_model advances v before yaw uses it.
"""
import json

import numpy as np
import pytest

from loop_checks import (EUNSUPPORTED, INF, check_assembled, check_solutions, dense, dev as _t, host, oracle_solve,
                         sim_qp as _sim_qp, stage_shift as _stage_shift)
from osqp_amd import canonical_data, mpc
from osqp_amd.mpc_device import IncrementalLayout

L_F, L_R, DT = 1.25, 1.40, 0.02  # simulate's vehicle (:238-251)
KIN = (mpc.KIN_Q, mpc.KIN_QN, mpc.KIN_R)
KIN_BOUNDS = (mpc.KIN_XMIN_T, mpc.KIN_XMAX_T, mpc.KIN_DUMIN, -mpc.KIN_DUMIN)


def _layout(N, **kw):
    return IncrementalLayout(N, *KIN, *KIN_BOUNDS, maskA=mpc.KIN_MASK_A, maskB=mpc.KIN_MASK_B, **kw)


def _qp(Ad, Bd, gd, xt, Xr, N):
    return mpc.incremental_qp(list(Ad), list(Bd), list(gd), xt, Xr, *KIN, N, *KIN_BOUNDS)


# ------------------------------------------------------------------ host restatements --
def reference_search(path_x, path_y, path_yaw, set_speed, pred_state, dt, N):
    """mpc_incre_kine_func.py:28-81: pred_state (4, N+1), speed in row 2 -> Xr (4, N+1)."""
    return mpc.reference_search_paths(path_x[None], path_y[None], path_yaw[None], None, [set_speed], pred_state.T[None],
                                      dt)[0]


def tail(sol, Ad0, Bd0, gd0, Xr, xt, cnt, N):
    """simulate's loop after the solve (:194-217 unpack, :382-428), without its aliasing:
    returns (row, dist, cnt, done, xt, pred, pdu) with row the trajectory entry
    (x, y, yaw, steer increment), pred (N+1, 6) and pdu (N+1, 2) stage-major.  When the stop
    rule fires (done) xt stays and pred / pdu are the unpacked solution."""
    nx, nu, nxa = 4, 2, 6
    S = sol[:(N + 1) * nxa].reshape(N + 1, nxa)          # pred_x~ as mpc_increment leaves it
    D = sol[(N + 1) * nxa:].reshape(N, nu)                # pred_del_u (its column N repeats N-1)
    u = xt[nx:] + D[0]
    x = Ad0 @ xt[:nx] + Bd0 @ u + gd0
    row = np.array([xt[0], xt[1], xt[3], D[0, 0]])
    dist = np.sqrt((Xr[0, 0] - xt[0]) ** 2 + (Xr[1, 0] - xt[1]) ** 2)
    if dist < 0.5:
        cnt = cnt + 1
        if cnt > 15:
            return row, dist, cnt, True, xt.copy(), S.copy(), np.vstack([D, D[-1:]])
    xt_new = np.concatenate([x, u])
    pred = np.empty((N + 1, nxa)); pdu = np.empty((N + 1, nu))
    pred[0] = xt_new
    pred[1:N] = S[2:N + 1]                                # columns 1 .. N-1 <- 2 .. N
    pdu[0:N - 1] = D[1:N]
    pdu[N - 1] = pdu[N] = D[N - 1]
    # terminal state: update_kinematics_model(column N's state, column N-1's control) -- and
    # column N-1 already holds column N.
    pred[N, :nx] = mpc.kin_update(L_F, L_R, DT, S[N, :nx], S[N, nx:])
    pred[N, nx:] = S[N, nx:]
    return row, dist, cnt, False, xt_new, pred, pdu


def rollout(x0, u0, N):
    """Initial guess (:289-308): the linearised model rolled forward with zero increments."""
    xk = np.concatenate([x0, u0], 1)
    pred = [xk]
    for i in range(N):
        Ad, Bd, gd = mpc.linearise_kinematics(L_F, L_R, DT, xk[:, :4], xk[:, 4:])
        xk = np.concatenate([np.einsum("bij,bj->bi", Ad, xk[:, :4]) + np.einsum("bij,bj->bi", Bd, xk[:, 4:]) + gd,
                             xk[:, 4:]], 1)
        pred.append(xk)
    return np.stack(pred, 1)                              # (B, N+1, 6)


def simulate(x0, path_x, path_y, path_yaw, N, max_steps, solve):
    """simulate (:223-436) for one vehicle with `solve(P, q, A, l, u) -> x`; returns
    (traj (rows x, y, yaw, steer increment), steps, dists)."""
    u0 = np.array([0.0, 0.01])
    xt = np.concatenate([x0, u0])
    pred = rollout(x0[None], u0[None], N)[0]
    traj = [np.array([x0[0], x0[1], x0[3], u0[1]])]       # :320-323 (traj_steer starts with u0[1, 0])
    cnt, dists = 0, []
    for step in range(max_steps):
        Xr = reference_search(path_x, path_y, path_yaw, x0[2], pred.T[:4], DT, N)
        Ad, Bd, gd = mpc.linearise_kinematics(L_F, L_R, DT, pred[:N, :4], pred[:N, 4:])
        sol = solve(*_qp(Ad, Bd, gd, xt, Xr, N))
        row, dist, cnt, done, xt, pred, _ = tail(sol, Ad[0], Bd[0], gd[0], Xr, xt, cnt, N)
        traj.append(row); dists.append(dist)
        if done:
            break
    return np.stack(traj), len(dists), np.array(dists)


_oracle_solve = oracle_solve(dict(polish=False, warm_start=False))


def _fixture_traj(g):
    return np.stack([g["traj_x"], g["traj_y"], g["traj_yaw"], g["traj_steer"]], 1)


# ----------------------------------------------------------------------- CPU tests --
def test_linearise_kinematics_matches_reference(golden):
    g = golden("kin_linearise.npz")
    assert (g["x"][:, 3] == 0).any() and (g["u"][:, 0] == 0).any() and (g["x"][:, 2] < 0).any()
    Ad, Bd, gd = mpc.linearise_kinematics(float(g["l_f"]), float(g["l_r"]), float(g["dt"]), g["x"], g["u"])
    assert np.allclose(Ad, g["Ad"], rtol=1e-13, atol=1e-15)
    assert np.allclose(Bd, g["Bd"], rtol=1e-13, atol=1e-15)
    assert np.allclose(gd, g["gd"], rtol=1e-13, atol=1e-15)
    # the masks are the structural nonzeros: nothing outside them, every entry of them hit somewhere
    assert not Ad[:, mpc.KIN_MASK_A == 0].any() and not Bd[:, mpc.KIN_MASK_B == 0].any()
    assert (Ad != 0).any(0)[mpc.KIN_MASK_A == 1].all() and (Bd != 0).any(0)[mpc.KIN_MASK_B == 1].all()


def test_reference_search_restatement_matches_reference(golden):
    g = golden("kin_refsearch.npz")
    N = g["pred"].shape[2] - 1
    assert g["path_yaw"].any() and (g["pred"][:, 2] < 0).all(1).sum() == g["pred"].shape[0] // 4
    for b in range(g["pred"].shape[0]):
        Xr = reference_search(g["path_x"], g["path_y"], g["path_yaw"], g["set_speed"][b], g["pred"][b],
                              float(g["dt"]), N)
        assert np.array_equal(Xr, g["Xr"][b])


def test_sim_steps_restatements_match_reference(golden):
    """Three steps of simulate as the reference ran them (kin_sim_n40.npz): the host
    restatements reproduce each step from its captured inputs and solution."""
    g = golden("kin_sim_n40.npz")
    N = 40
    assert np.allclose(g["in_pred"][0].T, rollout(g["x0"][None], g["in_xt"][0][None, 4:], N)[0], rtol=1e-12,
                       atol=1e-12)
    for t in range(g["in_xt"].shape[0]):
        pred = g["in_pred"][t].T                                  # (N+1, 6)
        Xr = reference_search(g["path_x"], g["path_y"], g["path_yaw"], g["x0"][2], pred.T[:4], DT, N)
        assert np.array_equal(Xr, g["in_Xr"][t])
        Ad, Bd, gd = mpc.linearise_kinematics(L_F, L_R, DT, pred[:N, :4], pred[:N, 4:])
        assert np.allclose(Ad, g["in_Ad"][t], rtol=1e-13, atol=1e-15)
        assert np.allclose(Bd, g["in_Bd"][t], rtol=1e-13, atol=1e-15)
        assert np.allclose(gd, g["in_gd"][t], rtol=1e-13, atol=1e-15)
        P, q, A, l, u = _qp(g["in_Ad"][t], g["in_Bd"][t], g["in_gd"][t], g["in_xt"][t], g["in_Xr"][t], N)
        Pr, qr, Ar, lr, ur = _sim_qp(g, t)
        assert np.array_equal(dense(P), dense(Pr)) and np.array_equal(dense(A), dense(Ar))
        assert np.array_equal(q, qr) and np.array_equal(l, lr) and np.array_equal(u, ur)
        row, dist, cnt, done, xt_new, pred_new, pdu_new = tail(g["sol"][t], g["in_Ad"][t][0], g["in_Bd"][t][0],
                                                               g["in_gd"][t][0], g["in_Xr"][t], g["in_xt"][t], 0, N)
        assert not done and cnt == int(dist < 0.5)
        assert np.allclose(xt_new, g["out_xt"][t], rtol=1e-12, atol=1e-12)
        assert np.allclose(pred_new, g["out_pred"][t].T, rtol=1e-12, atol=1e-12)
        assert np.allclose(pdu_new, g["out_pdu"][t].T, rtol=1e-12, atol=1e-12)
    # consecutive steps chain: a step's output is the next step's input
    assert np.array_equal(g["out_xt"][:-1], g["in_xt"][1:]) and np.array_equal(g["out_pred"][:-1], g["in_pred"][1:])
    assert np.array_equal(g["out_pdu"][:-1], g["in_pdu"][1:])


def test_whole_loop_restatement_matches_reference(golden):
    """The restated loop with the oracle solving stops where simulate stopped and leaves
    simulate's four trajectory lists (kin_stop_n40.npz)."""
    g = golden("kin_stop_n40.npz")
    traj, steps, dists = simulate(g["x0"], g["path_x"], g["path_y"], g["path_yaw"], 40, 200, _oracle_solve)
    assert steps == int(g["steps"]) and traj.shape[0] == steps + 1
    assert np.allclose(traj, _fixture_traj(g), rtol=1e-12, atol=1e-12)
    assert np.allclose(dists, g["dist"], rtol=1e-12, atol=1e-12)
    # the margin that makes the step count a fair thing to compare across solvers
    assert np.abs(g["dist"] - 0.5).min() > 2 * g["traj_sens"][0]


@pytest.mark.parametrize("N", [2, 3, 40])
def test_layout_pattern_matches_host_builder(N):
    L = _layout(N)
    P, A, lt, ut = L.pattern()
    assert (L.n, L.m) == ((N + 1) * 6 + N * 2, (N + 1) * 6 + (N + 1) * 6 + N * 2)
    P2, _, A2, l2, u2 = _qp([np.where(mpc.KIN_MASK_A, 7.0, 0.0)] * N, [np.where(mpc.KIN_MASK_B, 7.0, 0.0)] * N,
                            [np.zeros(4)] * N, np.zeros(6), np.zeros((4, N + 1)), N)
    P2, A2 = canonical_data(P2, A2)
    assert np.array_equal(P.indptr, P2.indptr) and np.array_equal(P.indices, P2.indices)
    assert np.array_equal(P.data, P2.data)
    assert np.array_equal(A.indptr, A2.indptr) and np.array_equal(A.indices, A2.indices)
    const = A2.data != 7.0
    assert np.array_equal(A.data[const], A2.data[const]) and not A.data[~const].any()
    ineq = slice((N + 1) * 6, None)
    assert np.array_equal(lt[ineq], np.clip(l2[ineq], -INF, INF))
    assert np.array_equal(ut[ineq], np.clip(u2[ineq], -INF, INF))


# ------------------------------------------------------------------------- GPU tests --
@pytest.mark.gpu
def test_kin_linearise_matches_reference_fixture(golden):
    import torch
    from osqp_amd.mpc_device import KinVehicle, linearise_kinematics
    g = golden("kin_linearise.npz")
    veh = KinVehicle(float(g["l_f"]), float(g["l_r"]), float(g["dt"]))
    x, u = _t(g["x"]), _t(g["u"])
    x0, u0 = x.clone(), u.clone()
    Ad, Bd, gd = linearise_kinematics(veh, x, u)
    assert torch.equal(x, x0) and torch.equal(u, u0)
    assert np.allclose(Ad.cpu().numpy(), g["Ad"], rtol=1e-13, atol=1e-15)
    assert np.allclose(Bd.cpu().numpy(), g["Bd"], rtol=1e-13, atol=1e-15)
    assert np.allclose(gd.cpu().numpy(), g["gd"], rtol=1e-13, atol=1e-15)
    # horizon-shaped input with a strided view: (B, N, 4) and (B, N, 2) taken from (B, N, 6)
    xt = torch.cat([x, u], dim=1).reshape(6, 8, 6)
    Ad3, Bd3, gd3 = linearise_kinematics(veh, xt[..., :4], xt[..., 4:])
    assert torch.equal(Ad3.reshape(48, 4, 4), Ad) and torch.equal(Bd3.reshape(48, 4, 2), Bd)
    assert torch.equal(gd3.reshape(48, 4), gd)


@pytest.mark.gpu
def test_kin_reference_search_matches_reference_fixture(golden):
    from osqp_amd.mpc_device import reference_search_kin
    g = golden("kin_refsearch.npz")
    pred = np.zeros((g["pred"].shape[0], g["pred"].shape[2], 6))
    pred[:, :, :4] = g["pred"].transpose(0, 2, 1)
    Xr = reference_search_kin(_t(g["path_x"]), _t(g["path_y"]), _t(g["path_yaw"]), _t(g["set_speed"]), _t(pred),
                              float(g["dt"])).cpu().numpy()
    assert np.array_equal(Xr, g["Xr"])
    # the path-end clamp (N = 10, B = 1): where the reference raises IndexError the kernel
    # holds the start of the last segment
    px, py, pyaw = g["path_x"], g["path_y"], g["path_yaw"]
    pred = np.zeros((1, 11, 6)); pred[0, :, 0] = 99.0; pred[0, :, 1] = -4.0; pred[0, :, 2] = 40.0
    Xr = reference_search_kin(_t(px), _t(py), _t(pyaw), _t([12.5]), _t(pred), 0.02).cpu().numpy()
    assert np.all(Xr[0, 0] == px[-2]) and np.all(Xr[0, 1] == py[-2])
    assert np.all(Xr[0, 2] == 12.5) and np.all(Xr[0, 3] == pyaw[-2])


def _kin_shift(L, veh, sol, Ad, Bd, gd, Xr, xt, pred, pdu, cnt, done, traj, cap, tlen):
    """mpcqp_kin_shift_device on device tensors, on the null stream; returns the call's code."""
    import ctypes as C
    import torch
    from osqp_amd.mpc_device import _bind, _p
    code = _bind().mpcqp_kin_shift_device(L._h, C.byref(veh), xt.shape[0], _p(sol), _p(Ad), _p(Bd), _p(gd), _p(Xr),
                                          _p(xt), _p(pred), _p(pdu), _p(cnt), _p(done), _p(traj), cap, _p(tlen),
                                          None)
    torch.cuda.synchronize()
    return code


@pytest.mark.gpu
def test_sim_steps_on_device_match_reference(golden):
    """Each captured step of simulate through every kernel against the reference's own values,
    and the device solve of the step's QP against the oracle's."""
    import torch
    import pyoracle
    from osqp_amd import OSQP
    from osqp_amd.mpc_device import KinVehicle, linearise_kinematics, reference_search_kin
    g = golden("kin_sim_n40.npz")
    N = 40
    T = g["in_xt"].shape[0]
    L, veh = _layout(N), KinVehicle()
    pred = _t(g["in_pred"].transpose(0, 2, 1))                   # (T, N+1, 6)
    Xr = reference_search_kin(_t(g["path_x"]), _t(g["path_y"]), _t(g["path_yaw"]), _t(np.full(T, g["x0"][2])), pred,
                              DT)
    assert np.array_equal(Xr.cpu().numpy(), g["in_Xr"])
    Ad, Bd, gd = linearise_kinematics(veh, pred[:, :N, :4], pred[:, :N, 4:])
    assert np.allclose(Ad.cpu().numpy(), g["in_Ad"], rtol=1e-13, atol=1e-15)
    assert np.allclose(Bd.cpu().numpy(), g["in_Bd"], rtol=1e-13, atol=1e-15)
    assert np.allclose(gd.cpu().numpy(), g["in_gd"], rtol=1e-13, atol=1e-15)
    Ax, q, l, u = L.assemble(_t(g["in_Ad"]), _t(g["in_Bd"]), _t(g["in_gd"]), _t(g["in_xt"]), _t(g["in_Xr"]))
    Apat = L.pattern()[1]
    for t in range(T):
        Pr, qr, Ar, lr, ur = _sim_qp(g, t)
        A_dev = Apat.copy(); A_dev.data = Ax[t].cpu().numpy()
        assert np.allclose(dense(A_dev), dense(Ar), rtol=1e-15, atol=0)
        assert np.allclose(q[t].cpu().numpy(), qr, rtol=1e-15, atol=0)
        assert np.array_equal(l[t].cpu().numpy(), np.clip(lr, -INF, INF))
        assert np.array_equal(u[t].cpu().numpy(), np.clip(ur, -INF, INF))
    # record, stop rule, plant step and shift of the captured solutions
    xt = _t(g["in_xt"]); pr = pred.clone(); pdu = _t(g["in_pdu"].transpose(0, 2, 1))
    cnt, done, tlen = (torch.zeros(T, dtype=torch.int32, device="cuda") for _ in range(3))
    traj = torch.zeros((T, 2, 4), dtype=torch.float64, device="cuda")
    keep = [_t(g[k]) for k in ("sol", "in_Ad", "in_Bd", "in_gd", "in_Xr")]
    assert _kin_shift(L, veh, *keep, xt, pr, pdu, cnt, done, traj, 2, tlen) == 0
    assert np.allclose(xt.cpu().numpy(), g["out_xt"], rtol=1e-12, atol=1e-12)
    assert np.allclose(pr.cpu().numpy(), g["out_pred"].transpose(0, 2, 1), rtol=1e-12, atol=1e-12)
    assert np.array_equal(pdu.cpu().numpy(), g["out_pdu"].transpose(0, 2, 1))
    near = np.hypot(g["in_Xr"][:, 0, 0] - g["in_xt"][:, 0], g["in_Xr"][:, 1, 0] - g["in_xt"][:, 1]) < 0.5
    assert np.array_equal(cnt.cpu().numpy(), near.astype(np.int32)) and not done.any() and (tlen == 1).all()
    du0 = g["sol"][:, (N + 1) * 6]
    assert np.array_equal(traj[:, 0].cpu().numpy(), np.stack([g["in_xt"][:, 0], g["in_xt"][:, 1], g["in_xt"][:, 3],
                                                              du0], 1))
    assert not traj[:, 1].any()
    # the solve of each captured QP: device and oracle agree, and the oracle reproduces the
    # solution the reference's loop ran on
    s = json.loads(str(g["settings"]))
    s.pop("verbose", None)
    for t in range(T):
        P, q_, A, l_, u_ = _sim_qp(g, t)
        o = pyoracle.OSQP(); o.setup(P, q_, A, l_, u_, **s); ro = o.solve()
        assert np.array_equal(ro.x, g["sol"][t]) and ro.info.iter == g["sol_iter"][t]
        d = OSQP(); d.setup(P, q_, A, l_, u_, **s); rd = d.solve()
        assert rd.info.status == ro.info.status and rd.info.iter == ro.info.iter
        assert np.abs(rd.x[(N + 1) * 6:] - ro.x[(N + 1) * 6:]).max() < 1e-4


def _test_path():
    px = np.linspace(-10, 100, 200)
    return px, px * 0.0 - 4.0, 0.02 * np.sin(px / 7.0)


@pytest.mark.gpu
def test_closed_loop_matches_host_restatement():
    import pyoracle
    from osqp_amd.mpc_device import KinematicMPC
    B, N, steps, cap = 5, 5, 6, 4
    x0 = np.zeros((B, 4))
    x0[:, 0] = [0.0, 3.0, 10.0, 20.0, 30.0]
    x0[:, 1] = [-3.7, -4.5, -2.5, -4.0, -4.2]                     # offsets from the path (y = -4)
    x0[:, 2] = [10.0, 15.0, 8.0, -6.0, 20.0]                      # vehicle 3 reverses
    x0[:, 3] = np.deg2rad([1.0, 5.0, -3.0, 10.0, 0.0])
    u0 = np.tile([0.0, 0.01], (B, 1)); u0[1, 0] = np.deg2rad(1.0)
    px, py, pyaw = _test_path()
    ctl = KinematicMPC(x0, u0, px, py, pyaw, N=N, traj_cap=cap)
    assert np.allclose(ctl.pred.cpu().numpy(), rollout(x0, u0, N), rtol=1e-12, atol=1e-12)
    Apat = ctl.layout.pattern()[1]
    n_iter_match = 0
    cnt = np.zeros(B, int)
    rows = [[np.array([x0[b, 0], x0[b, 1], x0[b, 3], u0[b, 1]])] for b in range(B)]
    for step in range(steps):
        xt, pred = ctl.xt.cpu().numpy(), ctl.pred.cpu().numpy()
        status, iters = ctl.step()
        status, iters = status.cpu().numpy(), iters.cpu().numpy()
        last, sol = host(ctl)
        for b in range(B):
            Xr = reference_search(px, py, pyaw, x0[b, 2], pred[b].T[:4], DT, N)
            assert np.array_equal(last["Xr"][b], Xr)
            Ad, Bd, gd = mpc.linearise_kinematics(L_F, L_R, DT, pred[b, :N, :4], pred[b, :N, 4:])
            P, q, A, l, u = _qp(Ad, Bd, gd, xt[b], Xr, N)
            check_assembled(last, b, Ad, Bd, gd, (P, q, A, l, u), Apat)
            o = pyoracle.OSQP()
            o.setup(P, q, A, l, u, polish=False, warm_start=False)
            ro = o.solve()
            assert status[b] == 1 and ro.info.status == "solved"
            n_iter_match += int(iters[b] == ro.info.iter)
            check_solutions(sol[b:b + 1], ro.x[None], slice((N + 1) * 6, None))
            # record, stop rule, plant step + shift from the device's own solution
            row, dist, cnt[b], done, xt_new, pred_new, pdu_new = tail(sol[b], last["Ad"][b, 0], last["Bd"][b, 0],
                                                                      last["gd"][b, 0], Xr, xt[b], cnt[b], N)
            assert not done
            rows[b].append(row)
            assert np.allclose(ctl.xt[b].cpu().numpy(), xt_new, rtol=1e-13, atol=1e-13)
            assert np.allclose(ctl.pred[b].cpu().numpy(), pred_new, rtol=1e-10, atol=1e-10)
            assert np.allclose(ctl.pdu[b].cpu().numpy(), pdu_new, rtol=0, atol=0)
    assert n_iter_match >= 0.9 * B * steps
    assert np.all(np.isfinite(ctl.xt.cpu().numpy()))
    assert np.array_equal(ctl.finish_cnt.cpu().numpy(), cnt) and not ctl.done.any()
    # the record holds the first traj_cap rows (initial state, then one per step) and stops there
    traj, tlen = ctl.trajectories()
    assert traj.shape == (B, cap, 4) and np.array_equal(tlen, np.full(B, cap))
    assert np.array_equal(traj, np.stack([np.stack(r[:cap]) for r in rows]))


@pytest.mark.gpu
def test_stop_and_freeze(golden):
    """Vehicles 0 and 2 run simulate's own case to its stop (kin_stop_n40.npz), vehicle 1 starts
    4 m off the path and keeps going.  A stopped vehicle stays as the stop left it while the
    batch steps on.  traj_len counts the lists' initial entry (:320-323), so after 60 steps
    the vehicle still running has 61 rows, as simulate's lists would."""
    from osqp_amd.mpc_device import KinematicMPC
    g = golden("kin_stop_n40.npz")
    ref = _fixture_traj(g)
    start = g["x0"]
    assert np.array_equal(start, [0.0, -3.7, 10.0, 0.02])
    x0 = np.stack([start, [0.0, 0.0, 10.0, 0.0], start])
    u0 = np.tile([0.0, 0.01], (3, 1))
    ctl = KinematicMPC(x0, u0, g["path_x"], g["path_y"], g["path_yaw"], N=40, traj_cap=64)
    assert ctl.run(60, check_every=4) == 60
    traj, tlen = ctl.trajectories()
    done, cnt = ctl.done.cpu().numpy(), ctl.finish_cnt.cpu().numpy()
    assert list(done) == [1, 0, 1] and cnt[0] == cnt[2] == 16
    assert tlen[0] == tlen[2] == ref.shape[0] == int(g["steps"]) + 1
    assert tlen[1] == 1 + 60
    for b in (0, 2):
        err = np.abs(traj[b, :tlen[b]] - ref).max(0)
        print("vehicle", b, "max |traj - fixture| per column", err, "traj_sens", g["traj_sens"])
        assert (err <= g["traj_sens"]).all(), (b, err, g["traj_sens"])
        assert not traj[b, tlen[b]:].any()
    assert np.array_equal(traj[0], traj[2])
    xt, pred, pdu = (v.cpu().numpy() for v in (ctl.xt, ctl.pred, ctl.pdu))
    assert np.array_equal(xt[0], xt[2]) and np.array_equal(pred[0], pred[2])
    # frozen since the stop: the state is still the last recorded one (step 49 of 60) ...
    for b in (0, 2):
        assert np.array_equal(xt[b, [0, 1, 3]], traj[b, tlen[b] - 1, :3])
    # ... and further steps leave everything of a stopped vehicle as it is
    for _ in range(2):
        ctl.step()
    xt2, pred2, pdu2 = (v.cpu().numpy() for v in (ctl.xt, ctl.pred, ctl.pdu))
    traj2, tlen2 = ctl.trajectories()
    for b in (0, 2):
        assert np.array_equal(xt2[b], xt[b]) and np.array_equal(pred2[b], pred[b]) and np.array_equal(pdu2[b], pdu[b])
        assert np.array_equal(traj2[b], traj[b]) and tlen2[b] == tlen[b]
    assert np.array_equal(ctl.finish_cnt.cpu().numpy()[[0, 2]], cnt[[0, 2]])
    assert tlen2[1] == 63 and not np.array_equal(xt2[1], xt[1])


@pytest.mark.gpu
def test_closed_loop_warm_start_matches_oracle():
    """warm_start=True (an extension): every step's solve starts from the previous solution
    shifted one stage; the oracle, warm-started from the same shifted iterates on the step's
    QP, gives the same controls.  Fewer iterations than the cold loop."""
    import pyoracle
    from osqp_amd.mpc_device import KinematicMPC
    B, N, steps = 16, 10, 5
    rng = np.random.default_rng(11)
    x0 = np.zeros((B, 4)); x0[:, 2] = rng.uniform(8, 20, B); x0[:, 1] = -4.0 + rng.uniform(-1.5, 1.5, B)
    x0[:, 3] = np.deg2rad(rng.uniform(-5, 5, B))
    u0 = np.tile([0.0, 0.01], (B, 1))
    px, py, pyaw = _test_path()
    cold = KinematicMPC(x0, u0, px, py, pyaw, N=N)
    warm = KinematicMPC(x0, u0, px, py, pyaw, N=N, warm_start=True)
    P, A, _, _ = warm.layout.pattern()
    Px = np.tile(P.data, (B, 1))
    du = slice((N + 1) * 6, None)
    ic = iw = match = 0
    prev = None
    for step in range(steps):
        sc, itc = cold.step()
        sw, itw = warm.step()
        ic += int(itc.sum()); iw += int(itw.sum())
        assert (sc.cpu().numpy() == 1).all() and (sw.cpu().numpy() == 1).all()
        last = {k: v.cpu().numpy() for k, v in warm.last.items()}
        ws = {} if prev is None else dict(x0=_stage_shift(prev[0], N, 6, 2, 1), y0=_stage_shift(prev[1], N, 6, 2, 2))
        ro = pyoracle.solve_batch(P, A, Px, last["q"], last["Ax"], last["l"], last["u"], nthreads=16, polish=False,
                                  **ws)
        x = warm.sol.cpu().numpy()
        same = ro.iter == itw.cpu().numpy()
        match += int(same.sum())
        assert np.abs(x[same][:, du] - ro.x[same][:, du]).max() < 1e-4
        prev = (x, warm.y.cpu().numpy())
    assert match >= 0.9 * B * steps
    assert iw < ic


@pytest.mark.gpu
def test_shift_entry_points_reject_the_other_model():
    """mpcqp_kin_shift_device takes only the nx 4 layout, mpcqp_incr_shift_device only nx 6."""
    import ctypes as C
    import torch
    from osqp_amd import lib
    from osqp_amd.mpc_device import KinVehicle, Vehicle, _bind, _p
    N, B = 4, 2
    L6 = IncrementalLayout(N, mpc.DYN_Q, mpc.DYN_QN, mpc.DYN_R, mpc.DYN_XMIN_T, mpc.DYN_XMAX_T, mpc.DYN_DUMIN,
                           -mpc.DYN_DUMIN)
    L4 = _layout(N)
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")
    zi = lambda: torch.zeros(B, dtype=torch.int32, device="cuda")
    # buffers sized for the larger model, so a call that wrongly went through stays in bounds
    sol, Ad, Bd, gd, Xr = z(B, L6.n), z(B, N, 6, 6), z(B, N, 6, 2), z(B, N, 6), z(B, 6, N + 1)
    xt, pred, pdu, traj = z(B, 8), z(B, N + 1, 8), z(B, N + 1, 2), z(B, 2, 4)
    assert _kin_shift(L6, KinVehicle(), sol, Ad, Bd, gd, Xr, xt, pred, pdu, zi(), zi(), traj, 2, zi()) == EUNSUPPORTED
    assert b"nx 4" in lib().mpcqp_last_error()
    code = _bind().mpcqp_incr_shift_device(L4._h, C.byref(Vehicle()), B, _p(sol), _p(Ad), _p(Bd), _p(gd), _p(xt),
                                           _p(pred), _p(pdu), None)
    torch.cuda.synchronize()
    assert code == EUNSUPPORTED
    assert not xt.any() and not pred.any()
