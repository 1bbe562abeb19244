"""Host-side MPC -> QP assembly and batch generators.

The reference assembles each QP with scipy.sparse before calling
osqp.OSQP().setup() (the boundary this package replaces):

  * lateral slack + incremental MPC   vehicle_lateral_mpc_slack_increment.py:32-121 (+ loop :126-229)
  * vanilla LTI MPC                    Control/MPC/mpc_kinematics.py:148-200 (`mpc`)
  * incremental LTV MPC                Control/MPC/mpc_dynamics.py:281-389 (`mpc_increment`),
                                       Control/MPC/mpc_increment_kinematics_pred_matrix.py:150-240
  * dynamic-bicycle linearisation      Vehicle_Dynamics/vehicle_models.py:52-340 (`get_dynamics_model`)

The builders here produce the same matrices (tests/test_assembly.py checks
them entry-for-entry against tests/golden/, captured from the reference) with
the variable order the reference uses, x = (x_0..x_N, u_0..u_{N-1}[, s_0..s_N]).
Batch generators (`make_batch`) vectorise the same formulas over B instances
that share one sparsity pattern -- the synthetic workloads of BASELINE.json's
configs.  Everything here is host numpy: data preparation,
not the solver.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sparse

# ------------------------------------------------------------------ models --
LATERAL_AD = np.array([[0.960, -0.019, 0., 0.],
                       [0.00469, 0.961, 0., 0.],
                       [0., 0.0196, 1., 0.],
                       [0.163, 0., 0.166, 1.]])          # slack script :32-37 (beta, r, e_psi, e_y)
LATERAL_BD = np.array([[0.020575], [0.115], [0.001157], [0.00182]])  # :39-43


def augment(Ad, Bd):
    """Incremental-input augmentation  x~ = [x; u_prev]:  A~ = [[Ad, Bd], [0, I]],  B~ = [Bd; I]
    (slack script :48-52, mpc_dynamics.py:333-361)."""
    nx, nu = Bd.shape
    At = np.block([[Ad, Bd], [np.zeros((nu, nx)), np.eye(nu)]])
    Bt = np.vstack([Bd, np.eye(nu)])
    return At, Bt


def _csc(M):
    M = sparse.csc_matrix(M)
    M.eliminate_zeros()
    M.sort_indices()
    return M


def _dyn_eq(Ad_list, Bd_list, N):
    """[-I stacked on the diagonal | A_k on the sub-diagonal | B_k shifted one block down]."""
    nx = Ad_list[0].shape[0]
    nu = Bd_list[0].shape[1]
    Ax = sparse.kron(sparse.eye(N + 1), -sparse.eye(nx), format="lil")
    Bu = sparse.lil_matrix(((N + 1) * nx, N * nu))
    for k in range(N):
        Ax[(k + 1) * nx:(k + 2) * nx, k * nx:(k + 1) * nx] = Ad_list[k]
        Bu[(k + 1) * nx:(k + 2) * nx, k * nu:(k + 1) * nu] = Bd_list[k]
    return sparse.hstack([Ax, Bu]).tocsc()


# ------------------------------------------------------- vanilla (cfg 2) --
def vanilla_qp(Ad, Bd, gd, x0, Xr, Q, QN, R, N, xmin, xmax, umin, umax):
    """Control/MPC/mpc_kinematics.py:148-191 (`mpc`): returns P, q, A, l, u."""
    Ad = np.asarray(Ad, float); Bd = np.asarray(Bd, float)
    nx, nu = Bd.shape
    Q = np.asarray(sparse.csr_matrix(Q).todense()); QN = np.asarray(sparse.csr_matrix(QN).todense())
    R = np.asarray(sparse.csr_matrix(R).todense())
    P = sparse.block_diag([sparse.kron(sparse.eye(N), Q), QN, sparse.kron(sparse.eye(N), R)])
    q = np.concatenate([-(Q @ Xr[:, k]) for k in range(N)] + [-(QN @ Xr[:, N]), np.zeros(N * nu)])
    Aeq = _dyn_eq([Ad] * N, [Bd] * N, N)
    gd = np.asarray(gd, float).ravel()
    leq = np.concatenate([-np.asarray(x0, float)] + [-gd] * N)
    Aineq = sparse.eye((N + 1) * nx + N * nu)
    lineq = np.concatenate([np.tile(xmin, N + 1), np.tile(umin, N)])
    uineq = np.concatenate([np.tile(xmax, N + 1), np.tile(umax, N)])
    A = sparse.vstack([Aeq, Aineq])
    return _csc(P), q, _csc(A), np.concatenate([leq, lineq]), np.concatenate([leq, uineq])


# ------------------------------------------------- LTV in the inputs themselves --
def ltv_qp(Ad_list, Bd_list, gd_list, x0, Xr, Q, QN, R, N, xmin, xmax, umin, umax, xlo=None, xhi=None):
    """The LTV MPC in (x_0..x_N, u_0..u_{N-1}) with per-stage Ad_k, Bd_k, gd_k:
    Control/MPC/mpc_kinematics_pred_matrix.py:268-352 (`mpc__`), Control/MPC/mpc_dynamics.py:160-279
    (`mpc`) and, with the per-stage state bounds xlo / xhi ((N+1, nx), replacing xmin / xmax),
    Control/MPC/mpc_kinematics.py:202-265 (`mpc_`, the x/y corridor).  Returns P, q, A, l, u."""
    Ad_list = [np.asarray(a, float) for a in Ad_list]
    Bd_list = [np.asarray(b, float) for b in Bd_list]
    nx, nu = Bd_list[0].shape
    if len(Ad_list) != N or len(Bd_list) != N or len(gd_list) != N:
        raise ValueError("Ad_list, Bd_list, gd_list must have N entries")
    Q = np.asarray(sparse.csr_matrix(Q).todense()); QN = np.asarray(sparse.csr_matrix(QN).todense())
    R = np.asarray(sparse.csr_matrix(R).todense())
    P = sparse.block_diag([sparse.kron(sparse.eye(N), Q), QN, sparse.kron(sparse.eye(N), R)])
    q = np.concatenate([-(Q @ Xr[:, k]) for k in range(N)] + [-(QN @ Xr[:, N]), np.zeros(N * nu)])
    Aeq = _dyn_eq(Ad_list, Bd_list, N)
    leq = np.concatenate([-np.asarray(x0, float).ravel()] + [-np.asarray(g, float).ravel() for g in gd_list])
    Aineq = sparse.eye((N + 1) * nx + N * nu)
    xl = np.tile(xmin, N + 1) if xlo is None else np.asarray(xlo, float).reshape((N + 1) * nx)
    xh = np.tile(xmax, N + 1) if xhi is None else np.asarray(xhi, float).reshape((N + 1) * nx)
    lineq = np.concatenate([xl, np.tile(umin, N)])
    uineq = np.concatenate([xh, np.tile(umax, N)])
    A = sparse.vstack([Aeq, Aineq])
    return _csc(P), q, _csc(A), np.concatenate([leq, lineq]), np.concatenate([leq, uineq])


# ---------------------------------------------------------- slack (cfg 1/3/4) --
SLACK_Q = np.diag([5., 5., 10., 10.])                        # :66
SLACK_R = 10.0                                               # :71
SLACK_W = np.array([10., 10., 10., 10., 0.])                 # :73 (0: the u_prev slot)
SLACK_WS = np.array([1., 1., 1., 1., 0.])                    # :104 slack coefficients
DEG = np.pi / 180.0


def slack_bounds(regime=0):
    """Bound schedule of the slack script :158-172 (regime 0: i<=400 / i>900, 1: 400<i<=900)."""
    dumin = np.array([-0.5 * DEG]); dumax = np.array([0.5 * DEG])
    xmin = np.array([-np.pi, -0.5 * np.pi, -15 * DEG, -10., -30 * DEG])
    xmax = np.array([np.pi, 0.5 * np.pi, 15 * DEG, 10., 30 * DEG])
    if regime == 1:
        xmin = xmin.copy(); xmin[3] = 2.0
    return xmin, xmax, dumin, dumax


def slack_qp(N, x0, xr=None, regime=0):
    """vehicle_lateral_mpc_slack_increment.py:48-115: soft-constrained incremental lateral MPC.
    Variables (x~_0..x~_N, du_0..du_{N-1}, s_0..s_N)."""
    At, Bt = augment(LATERAL_AD, LATERAL_BD)
    nx, nu = Bt.shape                                   # 5, 1
    nxs = nx - nu
    xr = np.zeros(nxs) if xr is None else np.asarray(xr, float)
    C = np.hstack([np.eye(nxs), np.zeros((nxs, nu))])
    Qt = C.T @ SLACK_Q @ C
    P = sparse.block_diag([sparse.kron(sparse.eye(N + 1), Qt), sparse.kron(sparse.eye(N), SLACK_R * np.eye(nu)),
                           sparse.kron(sparse.eye(N + 1), np.diag(SLACK_W))])
    qx = -(SLACK_Q @ C).T @ xr
    q = np.concatenate([np.tile(qx, N + 1), np.zeros(N * nu), np.zeros((N + 1) * nx)])
    Aeq = sparse.hstack([_dyn_eq([At] * N, [Bt] * N, N), sparse.csc_matrix(((N + 1) * nx, (N + 1) * nx))])
    Sineq = sparse.vstack([sparse.kron(sparse.eye(N + 1), np.diag(SLACK_WS)), sparse.csc_matrix((N * nu, (N + 1) * nx))])
    Aineq = sparse.hstack([sparse.eye((N + 1) * nx + N * nu), Sineq])
    xmin, xmax, dumin, dumax = slack_bounds(regime)
    leq = np.concatenate([-np.asarray(x0, float), np.zeros(N * nx)])
    lineq = np.concatenate([np.tile(xmin, N + 1), np.tile(dumin, N)])
    uineq = np.concatenate([np.tile(xmax, N + 1), np.tile(dumax, N)])
    A = sparse.vstack([Aeq, Aineq])
    return _csc(P), q, _csc(A), np.concatenate([leq, lineq]), np.concatenate([leq, uineq])


SLACK_SWITCH_STEPS = (400, 900)                              # :158-172: i <= 400 / i <= 900 / else
SLACK_REGIMES = (0, 1, 0)


def slack_regime(k, switch_steps=SLACK_SWITCH_STEPS, regimes=SLACK_REGIMES):
    """The bound regime step k assembles with (the script's if / elif / else, :158-172):
    regimes[#{j : k > switch_steps[j]}], elementwise over k."""
    k = np.asarray(k)
    r = sum((k > s).astype(np.int64) for s in switch_steps) if len(switch_steps) else np.zeros(k.shape, np.int64)
    return np.asarray(regimes, np.int32)[r]


def lti_step(At, Bt, sol, status, xt, step, regime, failed, fail_step, du_off, slack_off=-1,
             switch_steps=SLACK_SWITCH_STEPS, regimes=SLACK_REGIMES, traj=None, traj_len=None):
    """The tail of the slack script's loop (:252-269) for B vehicles: the arithmetic of
    mpc_device.hip::k_lti_step (mpcqp_lti_step_device) in numpy, in the kernel's operation order
    (elementwise numpy rounds every product and every sum on its own, as the kernel does).

    At (nxa, nxa), Bt (nxa, nu); sol (B, n) with du_0 = sol[:, du_off:du_off + nu] and the
    recorded slack sol[:, slack_off] (slack_off < 0: 0); status (B,) solver codes; xt (B, nxa);
    step, regime, failed, fail_step (B,) int32; traj (B, traj_cap, nxa + nu + 1) and traj_len (B,)
    or None.  Nothing is modified; returns (xt, step, regime, failed, fail_step, traj, traj_len).

    A failed vehicle is returned unchanged.  One whose status is not 1 (`solved`) gets failed = 1
    and fail_step = step -- the script's raise -- and is otherwise unchanged.  Every other one:
    record row (first nxa - nu states before the step, last nu after it, du_0, slack) while
    traj_len < traj_cap; x+ = At x + Bt du_0; step += 1; regime = slack_regime(step)."""
    At = np.asarray(At, float); Bt = np.asarray(Bt, float)
    nxa, nu = Bt.shape
    xt = np.array(xt, float); sol = np.asarray(sol, float)
    step, regime, failed, fail_step = (np.array(a, np.int32) for a in (step, regime, failed, fail_step))
    live = failed == 0
    bad = live & (np.asarray(status) != 1)
    go = live & ~bad
    fail_step[bad] = step[bad]
    failed[bad] = 1
    x = xt[:, :nxa]
    du = sol[:, du_off:du_off + nu]
    xn = np.empty_like(x)
    for i in range(nxa):
        acc = At[i, 0] * x[:, 0]
        for j in range(1, nxa):
            acc = acc + At[i, j] * x[:, j]
        bu = Bt[i, 0] * du[:, 0]
        for j in range(1, nu):
            bu = bu + Bt[i, j] * du[:, j]
        xn[:, i] = acc + bu
    if traj is not None:
        traj = np.array(traj, float); traj_len = np.array(traj_len, np.int32)
        slack = sol[:, slack_off] if slack_off >= 0 else np.zeros(len(xt))
        row = np.concatenate([x[:, :nxa - nu], xn[:, nxa - nu:], du, slack[:, None]], axis=1)
        rec = np.flatnonzero(go & (traj_len >= 0) & (traj_len < traj.shape[1]))
        traj[rec, traj_len[rec]] = row[rec]
        traj_len[rec] += 1
    xt[go, :nxa] = xn[go]
    step[go] += 1
    regime[go] = slack_regime(step[go], switch_steps, regimes)
    return xt, step, regime, failed, fail_step, traj, traj_len


# ------------------------------------------------------- incremental LTV (cfg 5) --
def incremental_qp(Ad_list, Bd_list, gd_list, xt0, Xr, Q, QN, R, N, xmin_t, xmax_t, dumin, dumax):
    """Control/MPC/mpc_dynamics.py:281-389 (`mpc_increment`): augmented LTV MPC in increments."""
    nx = Ad_list[0].shape[0]
    nu = Bd_list[0].shape[1]
    Q = np.asarray(sparse.csr_matrix(Q).todense()); QN = np.asarray(sparse.csr_matrix(QN).todense())
    R = np.asarray(sparse.csr_matrix(R).todense())
    C = np.hstack([np.eye(nx), np.zeros((nx, nu))])
    P = sparse.block_diag([sparse.kron(sparse.eye(N), C.T @ Q @ C), C.T @ QN @ C, sparse.kron(sparse.eye(N), R)])
    q = np.concatenate([-(Q @ C).T @ Xr[:, k] for k in range(N)] + [-(QN @ C).T @ Xr[:, N], np.zeros(N * nu)])
    aug = [augment(np.asarray(Ad_list[k], float), np.asarray(Bd_list[k], float)) for k in range(N)]
    Aeq = _dyn_eq([a[0] for a in aug], [a[1] for a in aug], N)
    gt = [np.concatenate([np.asarray(gd_list[k], float).ravel(), np.zeros(nu)]) for k in range(N)]
    leq = np.concatenate([-np.asarray(xt0, float)] + [-g for g in gt])
    Aineq = sparse.eye((N + 1) * (nx + nu) + N * nu)
    lineq = np.concatenate([np.tile(xmin_t, N + 1), np.tile(dumin, N)])
    uineq = np.concatenate([np.tile(xmax_t, N + 1), np.tile(dumax, N)])
    A = sparse.vstack([Aeq, Aineq])
    return _csc(P), q, _csc(A), np.concatenate([leq, lineq]), np.concatenate([leq, uineq])


# ------------------------------------------------ dynamic bicycle linearisation --
class VehicleParams:
    """Vehicle_Dynamics.__init__ (vehicle_models.py:27-50) defaults, dt as in mpc_dynamics.main (0.05)."""

    def __init__(self, m=1300, l_f=1.25, l_r=1.40, width=1.78, length=4.25, turning_circle=10.4,
                 C_d=0.34, A_f=2.0, C_roll=0.015, dt=0.05):
        self.m, self.l_f, self.l_r, self.dt = m, l_f, l_r, dt
        self.wheelbase = l_f + l_r
        self.Iz = 1 / 12 * m * (width ** 2 + length ** 2)
        self.C_d, self.A_f, self.C_roll, self.roh = C_d, A_f, C_roll, 1.23

    def pacejka(self):
        """Lateral Pacejka coefficients (vehicle_models.py:114-132): (B, C, D) front and rear."""
        a = [-22.1, 1011, 1078, 1.82, 0.208, 0.000, -0.354, 0.707]
        out = []
        for share in (self.l_r, self.l_f):
            Fz = 9.81 * (self.m * share / self.wheelbase) * 0.001
            C = 1.30
            D = a[0] * Fz ** 2 + a[1] * Fz
            BCD = a[2] * math.sin(a[3] * math.atan(a[4] * Fz))
            out.append((BCD / (C * D) * 180 / np.pi, C, D))
        return out


def linearise_dynamics(veh: VehicleParams, x, u):
    """Batched forward-Euler linearisation of the dynamic bicycle model
    (vehicle_models.py:52-340): x (B,6) = [X, Y, yaw, vx, vy, r], u (B,2) = [steer, accel]
    -> Ad (B,6,6), Bd (B,6,2), gd (B,6).  Applies the low-speed guard of :143-159
    to copies (the reference mutates the caller's arrays there)."""
    x = np.array(x, float, copy=True); u = np.array(u, float, copy=True)
    vx = x[:, 3]
    g1 = (vx >= 0) & (vx < 0.5)
    g2 = (vx > -0.5) & (vx < 0)
    g = g1 | g2
    x[g, 4] = 0.0; x[g, 5] = 0.0; u[g, 0] = 0.0
    x[g1 & (vx < 0.3), 3] = 0.3
    x[g2 & (vx > -0.3), 3] = -0.3
    (Bf, Cf, Df), (Br, Cr, Dr) = veh.pacejka()
    m, Iz, lf, lr = veh.m, veh.Iz, veh.l_f, veh.l_r
    yaw, vx, vy, r = x[:, 2], x[:, 3], x[:, 4], x[:, 5]
    st, acc = u[:, 0], u[:, 1]
    af = -np.arctan2(lf * r + vy, vx) + st
    ar = -np.arctan2(-lr * r + vy, vx)
    Fyf = Df * np.sin(Cf * np.arctan(Bf * af))
    Fyr = Dr * np.sin(Cr * np.arctan(Br * ar))
    R_roll = veh.C_roll * m * 9.81 * np.sign(vx)
    F_aero = 0.5 * veh.roh * veh.C_d * veh.A_f * vx ** 2 * np.sign(vx)
    Fx = m * acc - F_aero - R_roll
    cy, sy, cs, ss = np.cos(yaw), np.sin(yaw), np.cos(st), np.sin(st)
    f = np.stack([vx * cy - vy * sy, vy * cy + vx * sy, r,
                  1. / m * (Fx * cs - Fyf * ss + m * vy * r),
                  1. / m * (Fx * ss + Fyr + Fyf * cs - m * vx * r),
                  1. / Iz * (Fx * lf * ss + Fyf * lf * cs - Fyr * lr)], axis=1)
    dFx_dvx = -veh.roh * veh.C_d * veh.A_f * vx
    dFx_da = m
    kf = (Bf * Cf * Df * np.cos(Cf * np.arctan(Bf * af))) / (1 + Bf ** 2 * af ** 2)
    kr = (Br * Cr * Dr * np.cos(Cr * np.arctan(Br * ar))) / (1 + Br ** 2 * ar ** 2)
    nf = (lf * r + vy) ** 2 + vx ** 2
    nr = (-lr * r + vy) ** 2 + vx ** 2
    dFyf_dvx = kf * (lf * r + vy) / nf
    dFyf_dvy = kf * (-vx / nf)
    dFyf_dr = kf * (-lf * vx) / nf
    dFyf_dst = kf
    dFyr_dvx = kr * (-lr * r + vy) / nr
    dFyr_dvy = kr * (-vx) / nr
    dFyr_dr = kr * (lr * vx) / nr
    B = x.shape[0]
    Ac = np.zeros((B, 6, 6))
    Ac[:, 0, 2] = -vx * sy - vy * cy; Ac[:, 0, 3] = cy; Ac[:, 0, 4] = -sy
    Ac[:, 1, 2] = -vy * sy + vx * cy; Ac[:, 1, 3] = sy; Ac[:, 1, 4] = cy
    Ac[:, 2, 5] = 1.
    Ac[:, 3, 3] = 1 / m * (dFx_dvx * cs - dFyf_dvx * ss)
    Ac[:, 3, 4] = 1 / m * (-dFyf_dvy * ss + m * r)
    Ac[:, 3, 5] = 1 / m * (-dFyf_dr * ss + m * vy)
    Ac[:, 4, 3] = 1 / m * (dFx_dvx * ss + dFyr_dvx + dFyf_dvx * cs - m * r)
    Ac[:, 4, 4] = 1 / m * (dFyr_dvy + dFyf_dvy * cs)
    Ac[:, 4, 5] = 1 / m * (dFyr_dr + dFyf_dr * cs - m * vx)
    Ac[:, 5, 3] = 1 / Iz * (dFx_dvx * lf * ss + dFyf_dvx * lf * cs - dFyr_dvx * lr)
    Ac[:, 5, 4] = 1 / Iz * (dFyf_dvy * lf * cs - dFyr_dvy * lr)
    Ac[:, 5, 5] = 1 / Iz * (dFyf_dr * lf * cs - dFyr_dr * lr)
    Bc = np.zeros((B, 6, 2))
    Bc[:, 3, 0] = 1 / m * (-Fx * ss - dFyf_dst * ss - Fyf * cs)
    Bc[:, 3, 1] = 1 / m * (dFx_da * cs)
    Bc[:, 4, 0] = 1 / m * (Fx * cs + dFyf_dst * cs - Fyf * ss)
    Bc[:, 4, 1] = 1 / m * (dFx_da * ss)
    Bc[:, 5, 0] = 1 / Iz * (Fx * lf * cs + dFyf_dst * lf * cs - Fyf * lf * ss)
    Bc[:, 5, 1] = 1 / Iz * (dFx_da * lf * ss)
    gc = f - np.einsum("bij,bj->bi", Ac, x) - np.einsum("bij,bj->bi", Bc, u)
    Ad = np.eye(6)[None] + Ac * veh.dt
    return Ad, Bc * veh.dt, gc * veh.dt


# ---------------------------------------------- kinematic bicycle linearisation --
def linearise_kinematics(l_f, l_r, dt, x, u):
    """Batched Vehicle_Kinematics.get_kinematics_model (vehicle_models.py:835-863):
    x (B,4) = [X, Y, v, yaw], u (B,2) = [steer, accel] -> Ad (B,4,4), Bd (B,4,2), gd (B,4)
    (the reference's A, B, C: the model is already discrete)."""
    x = np.atleast_2d(np.asarray(x, float)); u = np.atleast_2d(np.asarray(u, float))
    wb = l_f + l_r
    v, yaw, st = x[:, 2], x[:, 3], u[:, 0]
    cy, sy, cs = np.cos(yaw), np.sin(yaw), np.cos(st)
    B = x.shape[0]
    Ad = np.tile(np.eye(4), (B, 1, 1))
    Ad[:, 0, 2] = dt * cy
    Ad[:, 0, 3] = -dt * v * sy
    Ad[:, 1, 2] = dt * sy
    Ad[:, 1, 3] = dt * v * cy
    Ad[:, 3, 2] = dt * np.tan(st) / wb
    Bd = np.zeros((B, 4, 2))
    Bd[:, 2, 1] = dt
    Bd[:, 3, 0] = dt * v / (wb * cs ** 2)
    gd = np.zeros((B, 4))
    gd[:, 0] = dt * v * sy * yaw
    gd[:, 1] = -dt * v * cy * yaw
    gd[:, 3] = -dt * v * st / (wb * cs ** 2)
    return Ad, Bd, gd


def kin_update(l_f, l_r, dt, x, u):
    """Vehicle_Kinematics.update_kinematics_model (vehicle_models.py:866-883) for x (.., 4), u (.., 2):
    the reference updates in place, so v advances before yaw reads it.  Returns the new state."""
    x, u = np.asarray(x, float), np.asarray(u, float)
    X, Y, v, yaw = x[..., 0], x[..., 1], x[..., 2], x[..., 3]
    v1 = v + u[..., 1] * dt
    return np.stack([X + v * np.cos(yaw) * dt, Y + v * np.sin(yaw) * dt, v1,
                     yaw + v1 / (l_f + l_r) * np.tan(u[..., 0]) * dt], axis=-1)


def per_vehicle(statement, vehicles, *batched, **common):
    """A statement of this module that takes ONE vehicle, over a fleet: vehicles[b] is the
    statement's leading argument(s) for vehicle b (a tuple is unpacked: (l_f, l_r, dt)); each of
    `batched` has the batch on axis 0 (None passes through) and vehicle b's call gets the slice
    [b:b+1], so the statement runs in its batch form on one vehicle; `common` goes to every call.
    Returns the statement's result(s) concatenated along axis 0: what B calls would give, stacked."""
    outs = []
    for b, v in enumerate(vehicles):
        lead = v if isinstance(v, tuple) else (v,)
        outs.append(statement(*lead, *(None if a is None else np.asarray(a)[b:b + 1] for a in batched), **common))
    if isinstance(outs[0], tuple):
        return tuple(np.concatenate([o[i] for o in outs]) for i in range(len(outs[0])))
    return np.concatenate(outs)


# ------------------------------------------- the MPC step differentiated (host) --
def _slots(M, rows, cols):
    """Positions in M.data (sorted CSC) of the entries (rows[i], cols[i]); -1 where not stored."""
    out = np.full(len(rows), -1, np.int64)
    for t, (r, c) in enumerate(zip(rows, cols)):
        lo, hi = M.indptr[c], M.indptr[c + 1]
        k = lo + np.searchsorted(M.indices[lo:hi], r)
        if k < hi and M.indices[k] == r:
            out[t] = k
    return out


def _take(g, slots):
    """g[:, slots] with zeros where the slot is -1."""
    return np.where(slots >= 0, g[:, np.maximum(slots, 0)], 0.0)


def _assemble_vjp(nxa, P, A, N, nx, nu, Q, QN, Xr, gPx, gAx, gq, gl, gu, xlo, xhi):
    """The transpose of ltv_qp (nxa = nx) / incremental_qp (nxa = nx + nu) in the order of
    mpc_assembly.hip's k_assemble_vjp_* (include/mpcqp.h, mpcqp_*_assemble_vjp_device)."""
    from types import SimpleNamespace
    A = sparse.csc_matrix(A); A.sort_indices()
    P = sparse.triu(sparse.csc_matrix(P), format="csc"); P.sort_indices()
    n, m, ns = P.shape[0], A.shape[0], (N + 1) * nxa
    given = [g for g in (gPx, gAx, gq, gl, gu) if g is not None]
    if not given:
        raise ValueError("at least one cotangent must be given")
    flat = all(np.ndim(g) == 1 for g in given)
    B = np.atleast_2d(given[0]).shape[0]

    def arr(g, w):
        return np.zeros((B, w)) if g is None else np.atleast_2d(np.asarray(g, float))

    gPx, gAx, gq, gl, gu = arr(gPx, P.nnz), arr(gAx, A.nnz), arr(gq, n), arr(gl, m), arr(gu, m)
    Q = np.asarray(sparse.csr_matrix(Q).todense(), float); QN = np.asarray(sparse.csr_matrix(QN).todense(), float)
    tr = nxa != nx
    W = (Q.T, QN.T) if tr else (Q, QN)                       # what the forward multiplies Xr_k with
    o = SimpleNamespace()
    # Ad_k[i][j] at (row (k+1) nxa + i, column k nxa + j); Bd_k[i][j] at column k nxa + nx + j (A~_k,
    # augmented layout only) and at column ns + k nu + j (B~_k)
    k, i, j = np.meshgrid(np.arange(N), np.arange(nx), np.arange(nx), indexing="ij")
    o.gAd = _take(gAx, _slots(A, ((k + 1) * nxa + i).ravel(), (k * nxa + j).ravel())).reshape(B, N, nx, nx)
    k, i, j = np.meshgrid(np.arange(N), np.arange(nx), np.arange(nu), indexing="ij")
    rows = ((k + 1) * nxa + i).ravel()
    gB = _take(gAx, _slots(A, rows, (ns + k * nu + j).ravel()))
    if tr:
        gB = _take(gAx, _slots(A, rows, (k * nxa + nx + j).ravel())) + gB
    o.gBd = gB.reshape(B, N, nx, nu)
    ge = -(gl + gu)
    o.ggd = np.ascontiguousarray(ge[:, nxa:ns].reshape(B, N, nxa)[:, :, :nx])
    o.gx0 = ge[:, :nxa].copy()
    gqs = gq[:, :ns].reshape(B, N + 1, nxa)
    o.gXr = np.empty((B, nx, N + 1))
    for kk in range(N + 1):
        Wk = W[1] if kk == N else W[0]
        for jj in range(nx):
            acc = np.zeros(B)
            for ii in range(nx):
                acc = acc + Wk[ii, jj] * gqs[:, kk, ii]
            o.gXr[:, jj, kk] = -acc
    INF = 1e30
    o.gxlo = o.gxhi = None
    if xlo is not None:
        x = np.asarray(xlo, float).reshape(-1, ns)
        o.gxlo = np.where((x > -INF) & (x < INF), gl[:, ns:2 * ns], 0.0).reshape(B, N + 1, nxa)
    if xhi is not None:
        x = np.asarray(xhi, float).reshape(-1, ns)
        o.gxhi = np.where((x > -INF) & (x < INF), gu[:, ns:2 * ns], 0.0).reshape(B, N + 1, nxa)
    # the weights: P's stored entry of stage k's W[i][j] (i <= j), stages ascending, minus the q part
    o.gQ, o.gQN, o.gR = np.zeros((B, nx, nx)), np.zeros((B, nx, nx)), np.zeros((B, nu, nu))
    Xr = None if Xr is None else np.asarray(Xr, float).reshape(-1, nx, N + 1)
    for ii in range(nx):
        for jj in range(nx):
            gi, xj = (jj, ii) if tr else (ii, jj)
            for out, stages in ((o.gQ, range(N)), (o.gQN, [N])):
                pp, qq = np.zeros(B), np.zeros(B)
                if ii <= jj:
                    for s in _slots(P, [kk * nxa + ii for kk in stages], [kk * nxa + jj for kk in stages]):
                        if s >= 0:
                            pp = pp + gPx[:, s]
                if Xr is not None:
                    for kk in stages:
                        qq = qq + gqs[:, kk, gi] * Xr[:, xj, kk]
                out[:, ii, jj] = pp - qq
    for ii in range(nu):
        for jj in range(ii, nu):
            pp = np.zeros(B)
            for s in _slots(P, [ns + kk * nu + ii for kk in range(N)], [ns + kk * nu + jj for kk in range(N)]):
                if s >= 0:
                    pp = pp + gPx[:, s]
            o.gR[:, ii, jj] = pp
    if flat:
        for key, v in vars(o).items():
            if v is not None:
                setattr(o, key, v[0])
    return o


def ltv_qp_vjp(P, A, N, nx, nu, Q, QN, Xr=None, gPx=None, gAx=None, gq=None, gl=None, gu=None, xlo=None, xhi=None):
    """The transpose of ltv_qp: cotangents on the stored values of triu(P) and A (sorted CSC, the
    patterns given -- the builder's or a layout's; an entry the pattern lacks has no gradient), on
    q, l and u, one instance (1-D) or a batch (leading axis) -> a namespace of gAd (N,nx,nx), gBd
    (N,nx,nu), ggd (N,nx), gx0 (nx), gXr (nx,N+1), gxlo / gxhi (N+1,nx; None without xlo / xhi:
    the forward's per-stage bounds, zero gradient where it clipped them to +-1e30), and gQ, gQN, gR
    with respect to the stored weights (include/mpcqp.h, mpcqp_ltv_assemble_vjp_device; Xr, the
    forward's, is read for gQ / gQN alone)."""
    return _assemble_vjp(nx, P, A, N, nx, nu, Q, QN, Xr, gPx, gAx, gq, gl, gu, xlo, xhi)


def incremental_qp_vjp(P, A, N, nx, nu, Q, QN, Xr=None, gPx=None, gAx=None, gq=None, gl=None, gu=None):
    """The transpose of incremental_qp, as ltv_qp_vjp: gx0 is gxt0 (nx+nu), gBd sums the two
    slots Bd_k has in A (A~_k's upper-right block, then B~_k), and q reads (Q C)', so gQ[i][j]
    takes gq[k nxa + j] Xr[i,k]."""
    return _assemble_vjp(nx + nu, P, A, N, nx, nu, Q, QN, Xr, gPx, gAx, gq, gl, gu, None, None)


def linearise_kinematics_vjp(l_f, l_r, dt, x, u, gAd, gBd, ggd):
    """The VJP of linearise_kinematics in the order of mpc_linearise.hip's k_kin_linearise_vjp:
    x (..., 4), u (..., 2), gAd (..., 4, 4), gBd (..., 4, 2), ggd (..., 4) -> gx (..., 4),
    gu (..., 2); only v, yaw and steer carry derivative."""
    x, u = np.asarray(x, float), np.asarray(u, float)
    gAd, gBd, ggd = np.asarray(gAd, float), np.asarray(gBd, float), np.asarray(ggd, float)
    wb = l_f + l_r
    v, yaw, st = x[..., 2], x[..., 3], u[..., 0]
    cy, sy, cs, ss = np.cos(yaw), np.sin(yaw), np.cos(st), np.sin(st)
    sec2, dsec2 = 1.0 / (cs * cs), 2.0 * ss / (cs * cs * cs)
    a02, a03, a12, a13, a32 = gAd[..., 0, 2], gAd[..., 0, 3], gAd[..., 1, 2], gAd[..., 1, 3], gAd[..., 3, 2]
    b30, g0, g1, g3 = gBd[..., 3, 0], ggd[..., 0], ggd[..., 1], ggd[..., 3]
    gx, gu = np.zeros(x.shape), np.zeros(u.shape)
    gx[..., 2] = dt * ((a13 * cy - a03 * sy) + (g0 * sy - g1 * cy) * yaw + (b30 - g3 * st) * sec2 / wb)
    gx[..., 3] = dt * ((a12 * cy - a02 * sy) - v * (a03 * cy + a13 * sy)
                       + v * (g0 * (cy * yaw + sy) + g1 * (sy * yaw - cy)))
    gu[..., 0] = dt / wb * (a32 * sec2 + v * (b30 * dsec2 - g3 * (sec2 + st * dsec2)))
    return gx, gu


class _Dual:
    """vehicle_model.h's Dual in numpy: a value v (...) and its tangent d (..., 6) in
    (yaw, vx, vy, r, steer, accel), with that struct's rules, operation by operation."""
    __array_ufunc__ = None  # ndarray op _Dual -> _Dual's reflected operator

    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def input(v, slot, live):
        d = np.zeros(v.shape + (6,))
        d[..., slot] = np.where(live, 1.0, 0.0)
        return _Dual(v, d)

    def __neg__(self):
        return _Dual(-self.v, -self.d)

    def __add__(self, o):
        return _Dual(self.v + o.v, self.d + o.d) if isinstance(o, _Dual) else _Dual(self.v + o, self.d)

    __radd__ = __add__

    def __sub__(self, o):
        return _Dual(self.v - o.v, self.d - o.d) if isinstance(o, _Dual) else _Dual(self.v - o, self.d)

    def __mul__(self, o):
        if isinstance(o, _Dual):
            return _Dual(self.v * o.v, self.d * o.v[..., None] + self.v[..., None] * o.d)
        return _Dual(self.v * o, self.d * (o[..., None] if isinstance(o, np.ndarray) else o))

    __rmul__ = __mul__

    def __truediv__(self, o):
        if not isinstance(o, _Dual):  # a plain value under a dual (the parameter statements only)
            return _Dual(self.v / o, self.d / (o[..., None] if isinstance(o, np.ndarray) else o))
        q = self.v / o.v
        return _Dual(q, (self.d - q[..., None] * o.d) / o.v[..., None])

    def __rtruediv__(self, o):  # a plain value over a dual
        q = o / self.v
        return _Dual(q, (-q[..., None] * self.d) / self.v[..., None])

    def chain(self, v, dv):
        return _Dual(v, dv[..., None] * self.d)

    def sin(self):
        return self.chain(np.sin(self.v), np.cos(self.v))

    def cos(self):
        return self.chain(np.cos(self.v), -np.sin(self.v))

    def atan(self):
        return self.chain(np.arctan(self.v), 1.0 / (1.0 + self.v * self.v))

    @staticmethod
    def atan2(y, x):
        n = x.v * x.v + y.v * y.v
        return _Dual(np.arctan2(y.v, x.v), (x.v[..., None] * y.d - y.v[..., None] * x.d) / n[..., None])


def linearise_dynamics_vjp(veh: VehicleParams, x, u, gAd=None, gBd=None, ggd=None):
    """The VJP of linearise_dynamics in the order of mpc_linearise.hip's k_linearise_vjp: x (..., 6),
    u (..., 2), cotangents gAd (..., 6, 6), gBd (..., 6, 2), ggd (..., 6) (None = zero) -> gx
    (..., 6), gu (..., 2).

    It differentiates the forward AS IT COMPUTES: the low-speed guard first (what it replaces by
    a constant carries no derivative: vy, r, steer for |vx| < 0.5, vx too for |vx| < 0.3), then
    f, Ac, Bc of get_dynamics_model over forward-mode duals in (yaw, vx, vy, r, steer, accel),
    each value's tangent taken with the weight of what the forward makes of it:
    Ad = I + dt Ac, Bd = dt Bc, gd = dt (f - Ac x - Bc u).  The reference's Ac is not everywhere
    the derivative of its f (dFx/dvx = -cda vx against -0.5 cda vx^2 sgn(vx)), so nothing cancels
    in gd; sgn(vx) has derivative 0.  X and Y never enter."""
    x, u = np.array(x, float, copy=True), np.array(u, float, copy=True)
    lead = x.shape[:-1]
    x, u = x.reshape(-1, 6), u.reshape(-1, 2)
    shape = x.shape[:-1]
    zero = lambda g, tail: np.zeros(shape + tail) if g is None else np.asarray(g, float).reshape(shape + tail)
    gAd, gBd, ggd = zero(gAd, (6, 6)), zero(gBd, (6, 2)), zero(ggd, (6,))
    vx_in = x[..., 3].copy()
    g1 = (vx_in >= 0) & (vx_in < 0.5)
    g2 = (vx_in > -0.5) & (vx_in < 0)
    gd_ = g1 | g2
    x[gd_, 4] = 0.0; x[gd_, 5] = 0.0; u[gd_, 0] = 0.0
    x[g1 & (vx_in < 0.3), 3] = 0.3
    x[g2 & (vx_in > -0.3), 3] = -0.3
    lat = ~((vx_in > -0.5) & (vx_in < 0.5))
    lon = ~((vx_in > -0.3) & (vx_in < 0.3))
    const = lambda v: _Dual(v, np.zeros(v.shape + (6,)))
    xd = [const(x[..., 0]), const(x[..., 1]), _Dual.input(x[..., 2], 0, True), _Dual.input(x[..., 3], 1, lon),
          _Dual.input(x[..., 4], 2, lat), _Dual.input(x[..., 5], 3, lat)]
    ud = [_Dual.input(u[..., 0], 4, lat), _Dual.input(u[..., 1], 5, True)]
    (Bf, Cf, Df), (Br, Cr, Dr) = veh.pacejka()
    m, Iz, lf, lr, dt = veh.m, veh.Iz, veh.l_f, veh.l_r, veh.dt
    cda, roll = veh.roh * veh.C_d * veh.A_f, veh.C_roll * m * 9.81
    yaw, vx, vy, r = xd[2:]
    st, acc = ud
    # tyre_forces
    af = -_Dual.atan2(lf * r + vy, vx) + st
    ar = -_Dual.atan2(-lr * r + vy, vx)
    Fyf = Df * (Cf * (Bf * af).atan()).sin()
    Fyr = Dr * (Cr * (Br * ar).atan()).sin()
    sg = np.sign(vx.v)
    Fx = m * acc - 0.5 * cda * vx * vx * sg - roll * sg
    # dynamics
    cy, sy, cs, ss = yaw.cos(), yaw.sin(), st.cos(), st.sin()
    f = [vx * cy - vy * sy, vy * cy + vx * sy, r,
         1. / m * (Fx * cs - Fyf * ss + m * vy * r),
         1. / m * (Fx * ss + Fyr + Fyf * cs - m * vx * r),
         1. / Iz * (Fx * lf * ss + Fyf * lf * cs - Fyr * lr)]
    # continuous_model
    dFx_dvx = -cda * vx
    dFx_da = m
    kf = (Bf * Cf * Df * (Cf * (Bf * af).atan()).cos()) / (1 + Bf * Bf * af * af)
    kr = (Br * Cr * Dr * (Cr * (Br * ar).atan()).cos()) / (1 + Br * Br * ar * ar)
    af_num, ar_num = lf * r + vy, -lr * r + vy
    nf, nr = af_num * af_num + vx * vx, ar_num * ar_num + vx * vx
    dFyf_dvx = kf * af_num / nf
    dFyf_dvy = kf * (-vx / nf)
    dFyf_dr = kf * (-lf * vx) / nf
    dFyf_dst = kf
    dFyr_dvx = kr * ar_num / nr
    dFyr_dvy = kr * (-vx) / nr
    dFyr_dr = kr * (lr * vx) / nr
    one = const(np.ones(shape))
    Ac = {(0, 2): -vx * sy - vy * cy, (0, 3): cy, (0, 4): -sy,
          (1, 2): -vy * sy + vx * cy, (1, 3): sy, (1, 4): cy,
          (2, 5): one,
          (3, 3): 1 / m * (dFx_dvx * cs - dFyf_dvx * ss),
          (3, 4): 1 / m * (-dFyf_dvy * ss + m * r),
          (3, 5): 1 / m * (-dFyf_dr * ss + m * vy),
          (4, 3): 1 / m * (dFx_dvx * ss + dFyr_dvx + dFyf_dvx * cs - m * r),
          (4, 4): 1 / m * (dFyr_dvy + dFyf_dvy * cs),
          (4, 5): 1 / m * (dFyr_dr + dFyf_dr * cs - m * vx),
          (5, 3): 1 / Iz * (dFx_dvx * lf * ss + dFyf_dvx * lf * cs - dFyr_dvx * lr),
          (5, 4): 1 / Iz * (dFyf_dvy * lf * cs - dFyr_dvy * lr),
          (5, 5): 1 / Iz * (dFyf_dr * lf * cs - dFyr_dr * lr)}
    Bc = {(3, 0): 1 / m * (-Fx * ss - dFyf_dst * ss - Fyf * cs), (3, 1): 1 / m * (dFx_da * cs),
          (4, 0): 1 / m * (Fx * cs + dFyf_dst * cs - Fyf * ss), (4, 1): 1 / m * (dFx_da * ss),
          (5, 0): 1 / Iz * (Fx * lf * cs + dFyf_dst * lf * cs - Fyf * lf * ss), (5, 1): 1 / Iz * (dFx_da * lf * ss)}
    # VjpFold: F, then A, then B, as continuous_model emits them
    g = np.zeros(shape + (6,))
    for i in range(6):
        g += (ggd[..., i] * dt)[..., None] * f[i].d
    for (i, j), v in Ac.items():
        g += (gAd[..., i, j] * dt)[..., None] * v.d
        g += (-(ggd[..., i] * dt))[..., None] * (v * xd[j]).d
    for (i, j), v in Bc.items():
        g += (gBd[..., i, j] * dt)[..., None] * v.d
        g += (-(ggd[..., i] * dt))[..., None] * (v * ud[j]).d
    gx, gu = np.zeros(shape + (6,)), np.zeros(shape + (2,))
    gx[..., 2] = g[..., 0]
    gx[..., 3] = np.where(lon, g[..., 1], 0.0)
    gx[..., 4] = np.where(lat, g[..., 2], 0.0)
    gx[..., 5] = np.where(lat, g[..., 3], 0.0)
    gu[..., 0] = np.where(lat, g[..., 4], 0.0)
    gu[..., 1] = g[..., 5]
    return gx.reshape(lead + (6,)), gu.reshape(lead + (2,))


# ------------------------------------------ the dynamic closed loop's tail and its VJP --
def _fn(name, a):
    """sin / cos / atan of an ndarray or a _Dual."""
    return getattr(a, name)() if isinstance(a, _Dual) else getattr(np, {"atan": "arctan"}.get(name, name))(a)


def _atan2(y, x):
    if isinstance(y, _Dual) and not isinstance(x, _Dual):  # duals in the constants over a plain point
        n = x * x + y.v * y.v
        return _Dual(np.arctan2(y.v, x), (x[..., None] * y.d) / n[..., None])
    return _Dual.atan2(y, x) if isinstance(x, _Dual) else np.arctan2(y, x)


def _low_speed_guard(x, u):
    """vehicle_model.h's low_speed_guard on copies of x (M, 6), u (M, 2); also the two regions
    as k_linearise_vjp names them: lat / lon False where vy, r, steer / vx became constants."""
    x, u = np.array(x, float, copy=True), np.array(u, float, copy=True)
    vx_in = x[:, 3].copy()
    g1 = (vx_in >= 0) & (vx_in < 0.5)
    g2 = (vx_in > -0.5) & (vx_in < 0)
    g = g1 | g2
    x[g, 4] = 0.0; x[g, 5] = 0.0; u[g, 0] = 0.0
    x[g1 & (vx_in < 0.3), 3] = 0.3
    x[g2 & (vx_in > -0.3), 3] = -0.3
    return x, u, ~((vx_in > -0.5) & (vx_in < 0.5)), ~((vx_in > -0.3) & (vx_in < 0.3))


def model_constants(veh: VehicleParams):
    """The thirteen constants the kernels read (vehicle_model.h's VehicleK, mpcqp_fleet_constants'
    order): (m, l_f, l_r, Iz, dt, cda, roll, B_f, C_f, D_f, B_r, C_r, D_r)."""
    (Bf, Cf, Df), (Br, Cr, Dr) = veh.pacejka()
    return (veh.m, veh.l_f, veh.l_r, veh.Iz, veh.dt, veh.roh * veh.C_d * veh.A_f, veh.C_roll * veh.m * 9.81,
            Bf, Cf, Df, Br, Cr, Dr)


def _euler_step(veh: VehicleParams, x, u):
    """vehicle_model.h's euler_step<T> from a GUARDED point: x, u lists of six / two ndarrays or
    _Duals -> the six components of x + dt f(x, u) (tyre_forces, dynamics, operation by operation)."""
    return _euler_step_k(model_constants(veh), x, u)


def _euler_step_k(k, x, u):
    """_euler_step over the thirteen constants k themselves: floats, or _Duals in the constants
    with a plain point (euler_step_pvjp)."""
    m, lf, lr, Iz, dt, cda, roll, Bf, Cf, Df, Br, Cr, Dr = k
    yaw, vx, vy, r = x[2:]
    st, acc = u
    af = -_atan2(lf * r + vy, vx) + st
    ar = -_atan2(-lr * r + vy, vx)
    Fyf = Df * _fn("sin", Cf * _fn("atan", Bf * af))
    Fyr = Dr * _fn("sin", Cr * _fn("atan", Br * ar))
    sg = np.sign(vx.v if isinstance(vx, _Dual) else vx)
    Fx = m * acc - 0.5 * cda * vx * vx * sg - roll * sg
    cy, sy, cs, ss = _fn("cos", yaw), _fn("sin", yaw), _fn("cos", st), _fn("sin", st)
    f = [vx * cy - vy * sy, vy * cy + vx * sy, r,
         1. / m * (Fx * cs - Fyf * ss + m * vy * r),
         1. / m * (Fx * ss + Fyr + Fyf * cs - m * vx * r),
         1. / Iz * (Fx * lf * ss + Fyf * lf * cs - Fyr * lr)]
    return [x[i] + f[i] * dt for i in range(6)]


def _kin_tail_args(N, nx, nxa, sol, Ad0, Bd0, x, mode=None):
    sol, x = np.asarray(sol, float), np.asarray(x, float)
    lead = x.shape[:-1]
    S = sol.reshape(-1, sol.shape[-1])
    M = S.shape[0]
    mode = np.zeros(M, int) if mode is None else np.broadcast_to(np.asarray(mode, int).reshape(-1), (M,))
    return (lead, M, S[:, :(N + 1) * nxa].reshape(M, N + 1, nxa), S[:, (N + 1) * nxa:].reshape(M, N, 2),
            np.asarray(Ad0, float).reshape(M, nx, nx), np.asarray(Bd0, float).reshape(M, nx, 2), x.reshape(M, nxa),
            mode)


def _plant_step(A0, B0, g0, x, uu):
    """plant_step's association: (sum_j A0[i, j] x[j] + sum_j B0[i, j] u[j]) + g0[i]."""
    M, nx, nu = x.shape[0], A0.shape[1], B0.shape[2]
    xn = np.empty((M, nx))
    for i in range(nx):
        acc = np.zeros(M)
        for j in range(nx):
            acc = acc + A0[:, i, j] * x[:, j]
        bu = np.zeros(M)
        for j in range(nu):
            bu = bu + B0[:, i, j] * uu[:, j]
        xn[:, i] = (acc + bu) + g0[:, i]
    return xn


def _plant_step_vjp(A0, B0, w):
    """(Ad0' w, Bd0' w) in the kernel's order of summation."""
    M, nx, nu = w.shape[0], A0.shape[1], B0.shape[2]
    ga, gb = np.empty((M, nx)), np.empty((M, nu))
    for j in range(nx):
        acc = np.zeros(M)
        for i in range(nx):
            acc = acc + A0[:, i, j] * w[:, i]
        ga[:, j] = acc
    for j in range(nu):
        acc = np.zeros(M)
        for i in range(nx):
            acc = acc + B0[:, i, j] * w[:, i]
        gb[:, j] = acc
    return ga, gb


def _cot(g, M, tail):
    return np.zeros((M,) + tail) if g is None else np.asarray(g, float).reshape((M,) + tail)


def incr_shift(veh: VehicleParams, N, sol, Ad0, Bd0, gd0, xt):
    """Plant step and horizon shift of mpc_dynamics.main (:578-617) -- mpc_device.hip::k_incr_shift
    (mpcqp_incr_shift_device) in numpy, operation by operation, for one vehicle or a batch.

    sol (..., (N+1) 8 + N 2) = (x~_0..x~_N, du_0..du_{N-1}); Ad0 (..., 6, 6), Bd0 (..., 6, 2),
    gd0 (..., 6) stage 0 of the linearisation; xt (..., 8) = x~ as the step started.  Returns
    (xt', pred', pdu'): xt' = ((Ad0 x + Bd0 u) + gd0, u) with u = u_prev + du_0; pred' (..., N+1, 8)
    = (xt', x~_2..x~_N, (euler_step(x_N, u_{N-1}), u_N)) -- u_k the input part of x~_k, the Euler
    step update_dynamics_model from the guarded point --; pdu' (..., N+1, 2) = (du_1..du_{N-1},
    du_{N-1}, du_{N-1})."""
    lead, M, X, D, A0, B0, x0, _ = _kin_tail_args(N, 6, 8, sol, Ad0, Bd0, xt)
    g0 = np.asarray(gd0, float).reshape(M, 6)
    uu = x0[:, 6:] + D[:, 0]
    xn = np.concatenate([_plant_step(A0, B0, g0, x0[:, :6], uu), uu], axis=1)
    pred, pdu = np.empty((M, N + 1, 8)), np.empty((M, N + 1, 2))
    pred[:, 0] = xn
    pred[:, 1:N] = X[:, 2:N + 1]
    pdu[:, 0:N - 1] = D[:, 1:N]
    pdu[:, N - 1] = pdu[:, N] = D[:, N - 1]
    xg, ug, _, _ = _low_speed_guard(X[:, N, :6], X[:, N - 1, 6:])
    xe = _euler_step(veh, [xg[:, i] for i in range(6)], [ug[:, 0], ug[:, 1]])
    pred[:, N, :6] = np.stack(xe, axis=1)
    pred[:, N, 6:] = pred[:, N - 1, 6:]
    return xn.reshape(lead + (8,)), pred.reshape(lead + (N + 1, 8)), pdu.reshape(lead + (N + 1, 2))


def incr_shift_vjp(veh: VehicleParams, N, sol, Ad0, Bd0, xt, gxt=None, gpred=None, gpdu=None):
    """The VJP of incr_shift in the order of mpc_device.hip's k_tail_vjp<DynamicIncrTail>
    (mpcqp_incr_shift_vjp_device): cotangents gxt (..., 8), gpred (..., N+1, 8), gpdu (..., N+1, 2)
    of (xt', pred', pdu') (None = zero); xt the value from BEFORE the step.  Returns (gsol, gAd0,
    gBd0, ggd0, gxt_before) with the shapes of (sol, Ad0, Bd0, gd0, xt).

    The transpose of the forward as it computes.  The plant step is bilinear: with w = gxt +
    gpred[0] the cotangent of xt', gAd0 = w_x x', gBd0 = w_x u', ggd0 = w_x, the cotangent of u is
    w_u + Bd0' w_x (it goes to xt's input part and to du_0), gxt_before's state part Ad0' w_x.
    The shift is copies: x~_k (2 <= k <= N) takes gpred[k-1], du_k (1 <= k <= N-1) gpdu[k-1];
    du_{N-1} also takes gpdu[N-1] and gpdu[N], x~_N's input part also gpred[N]'s, added in the
    order of the output index.  x~_0 and x~_1 get zero but for x~_{N-1}'s input part, which is the
    Euler step's control.  The terminal state is euler_step over forward-mode duals in (yaw, vx,
    vy, r, steer, accel) at the guarded point, seeds 0 where the guard put a constant (so those
    entries get exactly nothing from it), its tangents contracted with gpred[N]'s state part; X and
    Y pass through it with derivative 1."""
    lead, M, X, D, A0, B0, x0, _ = _kin_tail_args(N, 6, 8, sol, Ad0, Bd0, xt)
    gxt, gpred, gpdu = _cot(gxt, M, (8,)), _cot(gpred, M, (N + 1, 8)), _cot(gpdu, M, (N + 1, 2))
    w = gxt + gpred[:, 0]
    uu = x0[:, 6:] + D[:, 0]
    gA0 = w[:, :6, None] * x0[:, None, :6]
    gB0 = w[:, :6, None] * uu[:, None, :]
    gg0 = w[:, :6].copy()
    ga, gb = _plant_step_vjp(A0, B0, w[:, :6])
    gx0 = np.concatenate([ga, w[:, 6:] + gb], axis=1)
    gX, gD = np.zeros((M, N + 1, 8)), np.zeros((M, N, 2))
    gX[:, 2:N + 1] = gpred[:, 1:N]
    gD[:, 0] = gx0[:, 6:]
    gD[:, 1:N] = gpdu[:, 0:N - 1]
    gD[:, N - 1] = (gD[:, N - 1] + gpdu[:, N - 1]) + gpdu[:, N]
    gX[:, N, 6:] = gX[:, N, 6:] + gpred[:, N, 6:]
    # the terminal Euler step
    xg, ug, lat, lon = _low_speed_guard(X[:, N, :6], X[:, N - 1, 6:])
    const = lambda v: _Dual(v, np.zeros(v.shape + (6,)))
    xd = [const(xg[:, 0]), const(xg[:, 1]), _Dual.input(xg[:, 2], 0, True), _Dual.input(xg[:, 3], 1, lon),
          _Dual.input(xg[:, 4], 2, lat), _Dual.input(xg[:, 5], 3, lat)]
    ud = [_Dual.input(ug[:, 0], 4, lat), _Dual.input(ug[:, 1], 5, True)]
    xe = _euler_step(veh, xd, ud)
    we = gpred[:, N, :6]
    g = np.zeros((M, 6))
    for i in range(6):
        g = g + we[:, i, None] * xe[i].d
    ge = np.stack([we[:, 0], we[:, 1], g[:, 0], np.where(lon, g[:, 1], 0.0), np.where(lat, g[:, 2], 0.0),
                   np.where(lat, g[:, 3], 0.0)], axis=1)
    gX[:, N, :6] = gX[:, N, :6] + ge
    gX[:, N - 1, 6] = gX[:, N - 1, 6] + np.where(lat, g[:, 4], 0.0)
    gX[:, N - 1, 7] = gX[:, N - 1, 7] + g[:, 5]
    gsol = np.concatenate([gX.reshape(M, -1), gD.reshape(M, -1)], axis=1)
    return (gsol.reshape(lead + (gsol.shape[1],)), gA0.reshape(lead + (6, 6)), gB0.reshape(lead + (6, 2)),
            gg0.reshape(lead + (6,)), gx0.reshape(lead + (8,)))


# ------------------------------------------- the kinematic tails and their VJPs --
def kin_update_vjp(l_f, l_r, dt, x, u, w):
    """The transpose of kin_update in closed form (vehicle_model.h::kin_update_vjp): x (.., 4), u
    (.., 2) the point, w (.., 4) the cotangent of the new state -> (gx (.., 4), gu (.., 2)).  v
    enters yaw's row through v1 = v + accel dt, which the reference forms first."""
    x, u, w = np.asarray(x, float), np.asarray(u, float), np.asarray(w, float)
    v, yaw, st = x[..., 2], x[..., 3], u[..., 0]
    wb = l_f + l_r
    v1 = v + u[..., 1] * dt
    cy, sy, ts, cs = np.cos(yaw), np.sin(yaw), np.tan(st), np.cos(st)
    w0, w1, w2, w3 = (w[..., i] for i in range(4))
    gx = np.stack([w0, w1,
                   ((w0 * cy * dt + w1 * sy * dt) + w2) + w3 * ts * dt / wb,
                   (-w0 * v * sy * dt + w1 * v * cy * dt) + w3], axis=-1)
    gu = np.stack([w3 * v1 * dt / (wb * (cs * cs)), w2 * dt + w3 * dt * dt * ts / wb], axis=-1)
    return gx, gu


def kin_incr_shift(veh, N, sol, Ad0, Bd0, gd0, xt, mode=None, pred=None, pdu=None):
    """The plant step and in-place horizon shift that simulate (mpc_incre_kine_func.py:385-428) and
    mpc_increment_kinematics_pred_matrix.main (:442-472) share -- mpc_device.hip::kin_incr_step_shift
    in numpy, operation by operation, for one vehicle or a batch, with the masks of k_kin_shift.

    veh = (l_f, l_r, dt); sol (..., (N+1) 6 + N 2) = (x~_0..x~_N, du_0..du_{N-1}); Ad0 (..., 4, 4),
    Bd0 (..., 4, 2), gd0 (..., 4) stage 0 of the linearisation; xt (..., 6) = x~ as the step started.
    Returns (xt', pred', pdu').  mode 0 (the default): xt' = ((Ad0 x + Bd0 u) + gd0, u) with u =
    u_prev + du_0; pred' (..., N+1, 6) = (xt', x~_2..x~_N, (kin_update(x_N, u_N), u_N)); pdu'
    (..., N+1, 2) = (du_1..du_{N-1}, du_{N-1}, du_{N-1}).  mode 1 (done was set): xt and the given
    pred, pdu come back as they are.  mode 2 (the stop rule fired on this step): xt stays, pred' is
    the unpacked (x~_0..x~_N), pdu' = (du_0..du_{N-1}, du_{N-1})."""
    lead, M, X, D, A0, B0, x0, mode = _kin_tail_args(N, 4, 6, sol, Ad0, Bd0, xt, mode)
    g0 = np.asarray(gd0, float).reshape(M, 4)
    uu = x0[:, 4:] + D[:, 0]
    xn = np.concatenate([_plant_step(A0, B0, g0, x0[:, :4], uu), uu], axis=1)
    pn, dn = np.empty((M, N + 1, 6)), np.empty((M, N + 1, 2))
    pn[:, 0] = xn
    pn[:, 1:N] = X[:, 2:N + 1]
    dn[:, 0:N - 1] = D[:, 1:N]
    dn[:, N - 1] = dn[:, N] = D[:, N - 1]
    pn[:, N, :4] = kin_update(*veh, X[:, N, :4], X[:, N, 4:])
    pn[:, N, 4:] = X[:, N, 4:]
    m2 = mode == 2
    xn[m2], pn[m2], dn[m2] = x0[m2], X[m2], np.concatenate([D[m2], D[m2, -1:]], axis=1)
    m1 = mode == 1
    if m1.any():
        xn[m1] = x0[m1]
        pn[m1] = np.asarray(pred, float).reshape(M, N + 1, 6)[m1]
        dn[m1] = np.asarray(pdu, float).reshape(M, N + 1, 2)[m1]
    return xn.reshape(lead + (6,)), pn.reshape(lead + (N + 1, 6)), dn.reshape(lead + (N + 1, 2))


def kin_incr_shift_vjp(veh, N, sol, Ad0, Bd0, xt, gxt=None, gpred=None, gpdu=None, mode=None):
    """The VJP of kin_incr_shift in the order of mpc_device.hip's k_tail_vjp<KinIncrTail>
    (mpcqp_kin_shift_vjp_device): cotangents gxt (..., 6), gpred (..., N+1, 6), gpdu (..., N+1, 2)
    of (xt', pred', pdu') (None = zero); xt the value from BEFORE the step.  Returns (gsol, gAd0,
    gBd0, ggd0, gxt_before) with the shapes of (sol, Ad0, Bd0, gd0, xt).

    mode 0, with w = gxt + gpred[0]: gAd0 = w_x x', gBd0 = w_x u', ggd0 = w_x, the cotangent of u is
    w_u + Bd0' w_x (to xt's input part and to du_0), gxt_before's state part Ad0' w_x; x~_k
    (2 <= k <= N) takes gpred[k-1], du_k (1 <= k <= N-1) gpdu[k-1], du_{N-1} also gpdu[N-1] and
    gpdu[N] in that order; x~_N also takes gpred[N]'s input part and then kin_update_vjp of
    gpred[N]'s state part at (x_N, u_N), its own two parts.  mode 1: everything zero, gxt_before =
    gxt.  mode 2: x~_k takes gpred[k], du_k gpdu[k], du_{N-1} also gpdu[N]; gxt_before = gxt, the
    model outputs zero.  The cotangent of the previous pred / pdu (gpred / gpdu in mode 1, else
    zero) is not formed here."""
    lead, M, X, D, A0, B0, x0, mode = _kin_tail_args(N, 4, 6, sol, Ad0, Bd0, xt, mode)
    gxt, gpred, gpdu = _cot(gxt, M, (6,)), _cot(gpred, M, (N + 1, 6)), _cot(gpdu, M, (N + 1, 2))
    w = gxt + gpred[:, 0]
    uu = x0[:, 4:] + D[:, 0]
    gA0 = w[:, :4, None] * x0[:, None, :4]
    gB0 = w[:, :4, None] * uu[:, None, :]
    gg0 = w[:, :4].copy()
    ga, gb = _plant_step_vjp(A0, B0, w[:, :4])
    gx0 = np.concatenate([ga, w[:, 4:] + gb], axis=1)
    gX, gD = np.zeros((M, N + 1, 6)), np.zeros((M, N, 2))
    gX[:, 2:N + 1] = gpred[:, 1:N]
    gD[:, 0] = gx0[:, 4:]
    gD[:, 1:N] = gpdu[:, 0:N - 1]
    gD[:, N - 1] = (gD[:, N - 1] + gpdu[:, N - 1]) + gpdu[:, N]
    ge, gue = kin_update_vjp(*veh, X[:, N, :4], X[:, N, 4:], gpred[:, N, :4])
    gX[:, N, :4] = gX[:, N, :4] + ge
    gX[:, N, 4:] = (gX[:, N, 4:] + gpred[:, N, 4:]) + gue
    m2 = mode == 2
    gX[m2] = gpred[m2]
    gD[m2] = gpdu[m2, :N]
    gD[m2, N - 1] = gD[m2, N - 1] + gpdu[m2, N]
    m1 = mode == 1
    gX[m1], gD[m1] = 0.0, 0.0
    off = mode != 0
    gA0[off], gB0[off], gg0[off], gx0[off] = 0.0, 0.0, 0.0, gxt[off]
    gsol = np.concatenate([gX.reshape(M, -1), gD.reshape(M, -1)], axis=1)
    return (gsol.reshape(lead + (gsol.shape[1],)), gA0.reshape(lead + (4, 4)), gB0.reshape(lead + (4, 2)),
            gg0.reshape(lead + (4,)), gx0.reshape(lead + (6,)))


def kin_ltv_shift(veh, N, sol, Ad0, Bd0, gd0, x, mode=None, u=None, pred_x=None, pred_u=None):
    """The tail of mpc_kinematics_pred_matrix.main's loop (:534-563) -- mpc_device.hip::
    k_kin_ltv_shift in numpy, operation by operation, for one vehicle or a batch.

    veh = (l_f, l_r, dt); sol (..., (N+1) 4 + N 2) = (S_0..S_N, U_0..U_{N-1}); Ad0, Bd0, gd0 stage 0
    of the linearisation; x (..., 4) the state as the step started.  Returns (x', u', pred_x',
    pred_u'): x' = (Ad0 x + Bd0 U_0) + gd0, u' = U_0, pred_x' (..., N+1, 4) = (x', S_2..S_N,
    kin_update(S_N, U_{N-1})) -- the terminal control is stage N-1's --, pred_u' (..., N+1, 2) =
    (U_1..U_{N-1}, U_{N-1}, U_{N-1}).  mode 1 (status != solved): the given x, u, pred_x, pred_u
    come back as they are."""
    lead, M, S, U, A0, B0, x0, mode = _kin_tail_args(N, 4, 4, sol, Ad0, Bd0, x, mode)
    g0 = np.asarray(gd0, float).reshape(M, 4)
    xn = _plant_step(A0, B0, g0, x0, U[:, 0])
    un = U[:, 0].copy()
    px, pu = np.empty((M, N + 1, 4)), np.empty((M, N + 1, 2))
    px[:, 0] = xn
    px[:, 1:N] = S[:, 2:N + 1]
    px[:, N] = kin_update(*veh, S[:, N], U[:, N - 1])
    pu[:, 0:N - 1] = U[:, 1:N]
    pu[:, N - 1] = pu[:, N] = U[:, N - 1]
    m1 = mode != 0
    if m1.any():
        xn[m1] = x0[m1]
        un[m1] = np.asarray(u, float).reshape(M, 2)[m1]
        px[m1] = np.asarray(pred_x, float).reshape(M, N + 1, 4)[m1]
        pu[m1] = np.asarray(pred_u, float).reshape(M, N + 1, 2)[m1]
    return (xn.reshape(lead + (4,)), un.reshape(lead + (2,)), px.reshape(lead + (N + 1, 4)),
            pu.reshape(lead + (N + 1, 2)))


def kin_ltv_shift_vjp(veh, N, sol, Ad0, Bd0, x, gx=None, gu=None, gpred_x=None, gpred_u=None, mode=None):
    """The VJP of kin_ltv_shift in the order of mpc_device.hip's k_tail_vjp<KinLtvTail>
    (mpcqp_kin_ltv_shift_vjp_device): cotangents gx (..., 4), gu (..., 2), gpred_x (..., N+1, 4),
    gpred_u (..., N+1, 2) of (x', u', pred_x', pred_u') (None = zero); x from BEFORE the step.
    Returns (gsol, gAd0, gBd0, ggd0, gx_before).

    mode 0, with w = gx + gpred_x[0]: gAd0 = w x', gBd0 = w U_0', ggd0 = w, gx_before = Ad0' w,
    g U_0 = Bd0' w + gu; S_k (2 <= k <= N) takes gpred_x[k-1], U_k (1 <= k <= N-1) gpred_u[k-1],
    U_{N-1} also gpred_u[N-1] and gpred_u[N] in that order; kin_update_vjp of gpred_x[N] at
    (S_N, U_{N-1}) goes into S_N and, last, into U_{N-1}.  mode 1: everything zero, gx_before = gx;
    the cotangent of the previous u, pred_x, pred_u (gu, gpred_x, gpred_u) is not formed here."""
    lead, M, S, U, A0, B0, x0, mode = _kin_tail_args(N, 4, 4, sol, Ad0, Bd0, x, mode)
    gx, gu = _cot(gx, M, (4,)), _cot(gu, M, (2,))
    gpx, gpu = _cot(gpred_x, M, (N + 1, 4)), _cot(gpred_u, M, (N + 1, 2))
    w = gx + gpx[:, 0]
    gA0 = w[:, :, None] * x0[:, None, :]
    gB0 = w[:, :, None] * U[:, 0][:, None, :]
    gg0 = w.copy()
    gxb, gb = _plant_step_vjp(A0, B0, w)
    gS, gU = np.zeros((M, N + 1, 4)), np.zeros((M, N, 2))
    gS[:, 2:N + 1] = gpx[:, 1:N]
    gU[:, 0] = gb + gu
    gU[:, 1:N] = gpu[:, 0:N - 1]
    gU[:, N - 1] = (gU[:, N - 1] + gpu[:, N - 1]) + gpu[:, N]
    ge, gue = kin_update_vjp(*veh, S[:, N], U[:, N - 1], gpx[:, N])
    gS[:, N] = gS[:, N] + ge
    gU[:, N - 1] = gU[:, N - 1] + gue
    off = mode != 0
    gS[off], gU[off], gA0[off], gB0[off], gg0[off], gxb[off] = 0.0, 0.0, 0.0, 0.0, 0.0, gx[off]
    gsol = np.concatenate([gS.reshape(M, -1), gU.reshape(M, -1)], axis=1)
    return (gsol.reshape(lead + (gsol.shape[1],)), gA0.reshape(lead + (4, 4)), gB0.reshape(lead + (4, 2)),
            gg0.reshape(lead + (4,)), gxb.reshape(lead + (4,)))


# ----------------------------- gradients with respect to the vehicle's constants --
# DESIGN.md §25.  The statements of mpc_linearise.hip's four *_pvjp kernels and of
# mpcqp_vehicle_constants_vjp, operation by operation.  Coordinates: the thirteen constants the
# kernels read (model_constants' order) for the dynamic bicycle, (l_f, l_r, dt) for the kinematic
# one.  Each takes ONE vehicle; per_vehicle applies them to a fleet.
def _constant_duals(k, shape):
    """The constants k as _Duals seeded in their own slots: constant c has d[..., c] = 1."""
    out = []
    for c, v in enumerate(k):
        d = np.zeros(shape + (len(k),))
        d[..., c] = 1.0
        out.append(_Dual(np.full(shape, float(v)), d))
    return out


def _stage_sum(g):
    """g (M, N, W) -> (M, W): the device's stage sum, acc = 0, acc += g[:, s] for s = 0 .. N-1."""
    acc = np.zeros(g.shape[:1] + g.shape[2:])
    for s in range(g.shape[1]):
        acc = acc + g[:, s]
    return acc


def linearise_dynamics_pvjp(veh: VehicleParams, x, u, gAd=None, gBd=None, ggd=None):
    """d (Ad, Bd, gd of linearise_dynamics) / d the thirteen constants, contracted with the
    cotangents and summed over the stages, in the order of mpc_linearise.hip's k_linearise_pvjp:
    x (..., N, 6), u (..., N, 2), gAd (..., N, 6, 6), gBd (..., N, 6, 2), ggd (..., N, 6)
    (None = zero) -> gK (..., 13).

    linearise_dynamics_vjp's rules with the roles exchanged: the guard first, then f, Ac, Bc over
    duals in the CONSTANTS at a plain guarded point (an input the guard replaced is a constant
    either way).  Each value folds with weight c dt into its tangent and with weight c into dt's
    own slot (Ad = I + dt Ac, Bd = dt Bc, gd = dt (f - Ac x - Bc u)); no model value reads dt."""
    x, u = np.asarray(x, float), np.asarray(u, float)
    lead, N = x.shape[:-2], x.shape[-2]
    x, u = x.reshape(-1, 6), u.reshape(-1, 2)
    shape = x.shape[:-1]
    zero = lambda g, tail: np.zeros(shape + tail) if g is None else np.asarray(g, float).reshape(shape + tail)
    gAd, gBd, ggd = zero(gAd, (6, 6)), zero(gBd, (6, 2)), zero(ggd, (6,))
    x, u, _, _ = _low_speed_guard(x, u)
    kv = model_constants(veh)
    dt = kv[4]
    m, lf, lr, Iz, _, cda, roll, Bf, Cf, Df, Br, Cr, Dr = _constant_duals(kv, shape)
    xs, us = [x[:, i] for i in range(6)], [u[:, 0], u[:, 1]]
    yaw, vx, vy, r = xs[2:]
    st, acc = us
    # tyre_forces
    af = -_atan2(lf * r + vy, vx) + st
    ar = -_atan2(-lr * r + vy, vx)
    Fyf = Df * (Cf * (Bf * af).atan()).sin()
    Fyr = Dr * (Cr * (Br * ar).atan()).sin()
    sg = np.sign(vx)
    Fx = m * acc - 0.5 * cda * vx * vx * sg - roll * sg
    # dynamics
    cy, sy, cs, ss = np.cos(yaw), np.sin(yaw), np.cos(st), np.sin(st)
    f = [vx * cy - vy * sy, vy * cy + vx * sy, r,
         1. / m * (Fx * cs - Fyf * ss + m * vy * r),
         1. / m * (Fx * ss + Fyr + Fyf * cs - m * vx * r),
         1. / Iz * (Fx * lf * ss + Fyf * lf * cs - Fyr * lr)]
    # continuous_model
    dFx_dvx = -cda * vx
    dFx_da = m
    kf = (Bf * Cf * Df * (Cf * (Bf * af).atan()).cos()) / (1 + Bf * Bf * af * af)
    kr = (Br * Cr * Dr * (Cr * (Br * ar).atan()).cos()) / (1 + Br * Br * ar * ar)
    af_num, ar_num = lf * r + vy, -lr * r + vy
    nf, nr = af_num * af_num + vx * vx, ar_num * ar_num + vx * vx
    dFyf_dvx = kf * af_num / nf
    dFyf_dvy = kf * (-vx / nf)
    dFyf_dr = kf * (-lf * vx) / nf
    dFyf_dst = kf
    dFyr_dvx = kr * ar_num / nr
    dFyr_dvy = kr * (-vx) / nr
    dFyr_dr = kr * (lr * vx) / nr
    Ac = {(0, 2): -vx * sy - vy * cy, (0, 3): cy, (0, 4): -sy,
          (1, 2): -vy * sy + vx * cy, (1, 3): sy, (1, 4): cy,
          (2, 5): np.ones(shape),
          (3, 3): 1 / m * (dFx_dvx * cs - dFyf_dvx * ss),
          (3, 4): 1 / m * (-dFyf_dvy * ss + m * r),
          (3, 5): 1 / m * (-dFyf_dr * ss + m * vy),
          (4, 3): 1 / m * (dFx_dvx * ss + dFyr_dvx + dFyf_dvx * cs - m * r),
          (4, 4): 1 / m * (dFyr_dvy + dFyf_dvy * cs),
          (4, 5): 1 / m * (dFyr_dr + dFyf_dr * cs - m * vx),
          (5, 3): 1 / Iz * (dFx_dvx * lf * ss + dFyf_dvx * lf * cs - dFyr_dvx * lr),
          (5, 4): 1 / Iz * (dFyf_dvy * lf * cs - dFyr_dvy * lr),
          (5, 5): 1 / Iz * (dFyf_dr * lf * cs - dFyr_dr * lr)}
    Bc = {(3, 0): 1 / m * (-Fx * ss - dFyf_dst * ss - Fyf * cs), (3, 1): 1 / m * (dFx_da * cs),
          (4, 0): 1 / m * (Fx * cs + dFyf_dst * cs - Fyf * ss), (4, 1): 1 / m * (dFx_da * ss),
          (5, 0): 1 / Iz * (Fx * lf * cs + dFyf_dst * lf * cs - Fyf * lf * ss), (5, 1): 1 / Iz * (dFx_da * lf * ss)}
    # PvjpFold: F, then A, then B, as continuous_model emits them
    g, gdt = np.zeros(shape + (13,)), np.zeros(shape)

    def fold(o, c):
        nonlocal g, gdt
        if isinstance(o, _Dual):
            g = g + (c * dt)[..., None] * o.d
            gdt = gdt + c * o.v
        else:
            gdt = gdt + c * o

    for i in range(6):
        fold(f[i], ggd[..., i])
    for (i, j), v in Ac.items():
        fold(v, gAd[..., i, j])
        fold(v * xs[j], -ggd[..., i])
    for (i, j), v in Bc.items():
        fold(v, gBd[..., i, j])
        fold(v * us[j], -ggd[..., i])
    g[..., 4] = gdt
    return _stage_sum(g.reshape(-1, N, 13)).reshape(lead + (13,))


def linearise_kinematics_pvjp(l_f, l_r, dt, x, u, gAd=None, gBd=None, ggd=None):
    """The same for linearise_kinematics, in closed form as k_kin_linearise_pvjp has it: x (..., N, 4),
    u (..., N, 2), gAd (..., N, 4, 4), gBd (..., N, 4, 2), ggd (..., N, 4) (None = zero) -> gK (..., 3)
    in (l_f, l_r, dt).  Every structural entry is dt times a function of the point and 1 / wb,
    wb = l_f + l_r, so l_f and l_r take the same value."""
    x, u = np.asarray(x, float), np.asarray(u, float)
    lead, N = x.shape[:-2], x.shape[-2]
    shape = x.shape[:-1]
    zero = lambda g, tail: np.zeros(shape + tail) if g is None else np.asarray(g, float).reshape(shape + tail)
    gAd, gBd, ggd = zero(gAd, (4, 4)), zero(gBd, (4, 2)), zero(ggd, (4,))
    wb = l_f + l_r
    v, yaw, st = x[..., 2], x[..., 3], u[..., 0]
    cy, sy, cs, ts = np.cos(yaw), np.sin(yaw), np.cos(st), np.tan(st)
    sec2 = 1.0 / (cs * cs)
    a02, a03, a12, a13, a32 = gAd[..., 0, 2], gAd[..., 0, 3], gAd[..., 1, 2], gAd[..., 1, 3], gAd[..., 3, 2]
    b21, b30, g0, g1, g3 = gBd[..., 2, 1], gBd[..., 3, 0], ggd[..., 0], ggd[..., 1], ggd[..., 3]
    over_wb = a32 * ts + (b30 - g3 * st) * v * sec2  # what 1 / wb multiplies, without dt
    gwb = -(dt * over_wb) / (wb * wb)
    gdt = ((a02 * cy + a12 * sy) + v * (a13 * cy - a03 * sy)) + b21 + v * yaw * (g0 * sy - g1 * cy) + over_wb / wb
    s = _stage_sum(np.stack([gwb, gdt], axis=-1).reshape(-1, N, 2))
    return np.stack([s[:, 0], s[:, 0], s[:, 1]], axis=-1).reshape(lead + (3,))


def euler_step_pvjp(veh: VehicleParams, x, u, w, mode=None):
    """d (the guarded Euler step _euler_step of x (..., 6), u (..., 2)) / d the thirteen
    constants, contracted with w (..., 6) -> gK (..., 13) (mpc_linearise.hip's k_euler_step_pvjp):
    the step over duals in the constants, dt among them, from the guarded plain point.  mode
    (...) or None: a vehicle whose mode is not 0 did not take the step and gets a zero row."""
    x, u, w = np.asarray(x, float), np.asarray(u, float), np.asarray(w, float)
    lead = x.shape[:-1]
    x, u, w = x.reshape(-1, 6), u.reshape(-1, 2), w.reshape(-1, 6)
    xg, ug, _, _ = _low_speed_guard(x, u)
    k = _constant_duals(model_constants(veh), xg.shape[:1])
    xe = _euler_step_k(k, [xg[:, i] for i in range(6)], [ug[:, 0], ug[:, 1]])
    g = np.zeros(xg.shape[:1] + (13,))
    for i in range(6):
        g = g + w[:, i, None] * xe[i].d
    if mode is not None:
        g[np.asarray(mode).reshape(-1) != 0] = 0.0
    return g.reshape(lead + (13,))


def kin_update_pvjp(l_f, l_r, dt, x, u, w, mode=None):
    """The same for kin_update in closed form (k_kin_update_pvjp): x (..., 4), u (..., 2), w (..., 4)
    -> gK (..., 3) in (l_f, l_r, dt)."""
    x, u, w = np.asarray(x, float), np.asarray(u, float), np.asarray(w, float)
    v, yaw, st, acc = x[..., 2], x[..., 3], u[..., 0], u[..., 1]
    wb = l_f + l_r
    v1 = v + acc * dt
    cy, sy, ts = np.cos(yaw), np.sin(yaw), np.tan(st)
    w0, w1, w2, w3 = (w[..., i] for i in range(4))
    gwb = -(w3 * v1 * ts * dt) / (wb * wb)
    gdt = (v * (w0 * cy + w1 * sy) + w2 * acc) + w3 * ts * (acc * dt + v1) / wb
    g = np.stack([gwb, gwb, gdt], axis=-1)
    if mode is not None:
        g[np.asarray(mode) != 0] = 0.0
    return g


def vehicle_constants(p):
    """The thirteen constants of the nine constructor arguments p = (m, l_f, l_r, width, length,
    C_d, A_f, C_roll, dt) (mpcqp_vehicle's field order), with vehicle_model.h's derivation
    operation by operation; floats, or _Duals in the arguments."""
    m, l_f, l_r, width, length, C_d, A_f, C_roll, dt = p
    Iz = 1.0 / 12 * m * (width * width + length * length)
    cda = 1.23 * C_d * A_f
    roll = C_roll * m * 9.81
    a = [-22.1, 1011, 1078, 1.82, 0.208, 0.000, -0.354, 0.707]
    wheelbase = l_f + l_r
    tyre = []
    for share in (l_r, l_f):
        Fz = 9.81 * (m * share / wheelbase) * 0.001
        C = 1.30
        D = a[0] * Fz * Fz + a[1] * Fz
        BCD = a[2] * _fn("sin", a[3] * _fn("atan", a[4] * Fz))
        tyre += [BCD / (C * D) * 180 / np.pi, C, D]
    return [m, l_f, l_r, Iz, dt, cda, roll] + tyre


def vehicle_constants_vjp(params, gk):
    """mpcqp_vehicle_constants_vjp: params (..., 9) the constructor arguments, gk (..., 13) the
    cotangent of the constants -> (..., 9), the transpose of vehicle_constants' Jacobian at
    params, formed by running vehicle_constants over duals in the nine arguments."""
    params, gk = np.asarray(params, float), np.asarray(gk, float)
    lead = params.shape[:-1]
    p = _constant_duals_of(params)
    k = vehicle_constants(p)
    g = np.zeros(lead + (9,))
    for c in range(13):
        if isinstance(k[c], _Dual):  # C_f, C_r are the number 1.30
            g = g + gk[..., c, None] * k[c].d
    return g


def _constant_duals_of(params):
    """params (..., 9) as nine _Duals, argument a seeded in slot a."""
    out = []
    for a in range(params.shape[-1]):
        d = np.zeros(params.shape)
        d[..., a] = 1.0
        out.append(_Dual(params[..., a], d))
    return out


# ------------------------------------------------------------ batch generators --
CONFIGS = {
    1: dict(name="slack-single-N20", layout="slack", N=20, B=1),
    2: dict(name="vanilla-lateral-N20", layout="vanilla", N=20, B=1024),
    3: dict(name="slack-lateral-N20", layout="slack", N=20, B=65536),
    4: dict(name="slack-lateral-N20-8gpu", layout="slack", N=20, B=262144),
    5: dict(name="incremental-dynamic-N50", layout="dynamic", N=50, B=8192),
}

VANILLA_Q = np.diag([5., 5., 10., 10.])
VANILLA_R = np.array([[10.]])
VANILLA_XMIN = np.array([-np.pi, -0.5 * np.pi, -15 * DEG, -10.])
VANILLA_UMAX = np.array([30 * DEG])

DYN_Q = np.diag([100.0, 100.0, 100.0, 50.0, 50.0, 50.0])        # mpc_dynamics.py:456-458
DYN_QN = np.diag([1000.0, 1000.0, 1000.0, 500.0, 500.0, 500.0])
DYN_R = np.diag([50., 50.])
DYN_DUMIN = np.array([-np.deg2rad(2.0), -0.5])                   # :461-464
DYN_XMIN_T = np.array([-np.inf, -np.inf, -2 * np.pi, -100., -30., -0.5 * np.pi, -np.deg2rad(15), -3.])
DYN_XMAX_T = np.array([np.inf, np.inf, 2 * np.pi, 100., 30., 0.5 * np.pi, np.deg2rad(15), 1.])

KIN_Q = np.diag([100.0, 100.0, 10.0, 100.0])                     # mpc_incre_kine_func.py:264-267
KIN_QN = np.diag([1000.0, 1000.0, 100.0, 1000.0])
KIN_R = np.diag([100., 100.])
KIN_DUMIN = np.array([-np.deg2rad(0.5), -0.5])                   # :257-260
KIN_XMIN_T = np.array([-np.inf, -np.inf, -100., -2 * np.pi, -np.deg2rad(15), -3.])
KIN_XMAX_T = np.array([np.inf, np.inf, 100., 2 * np.pi, np.deg2rad(15), 1.])
# structural nonzeros of get_kinematics_model's A and B (vehicle_models.py:843-856)
KIN_MASK_A = np.eye(4, dtype=np.uint8)
for _i, _j in [(0, 2), (0, 3), (1, 2), (1, 3), (3, 2)]:
    KIN_MASK_A[_i, _j] = 1
KIN_MASK_B = np.zeros((4, 2), np.uint8)
KIN_MASK_B[2, 1] = KIN_MASK_B[3, 0] = 1

KINLTV_Q = np.diag([10.0, 10.0, 100.0, 10.0])                    # mpc_kinematics_pred_matrix.py:425-435
KINLTV_QN = np.diag([100.0, 100.0, 1000.0, 100.0])
KINLTV_R = np.diag([1000., 100.])
KINLTV_UMIN = np.array([-np.deg2rad(15), -3.])
KINLTV_UMAX = np.array([np.deg2rad(15), 1.])
KINLTV_XMIN = np.array([-np.inf, -np.inf, -100., -2 * np.pi])
KINLTV_XMAX = np.array([np.inf, np.inf, 100., 2 * np.pi])

# mpc_increment_kinematics_pred_matrix.py:302-312 (the lane-change loop): KIN_*'s bounds, R and
# QN; only Q differs (50, 50, 10, 50 against 100, 100, 10, 100)
LANE_Q = np.diag([50.0, 50.0, 10.0, 50.0])
LANE_QN = np.diag([1000.0, 1000.0, 100.0, 1000.0])
LANE_R = np.diag([100., 100.])
LANE_DUMIN = np.array([-np.deg2rad(0.5), -0.5])
LANE_XMIN_T = np.array([-np.inf, -np.inf, -100., -2 * np.pi, -np.deg2rad(15), -3.])
LANE_XMAX_T = np.array([np.inf, np.inf, 100., 2 * np.pi, np.deg2rad(15), 1.])
LANE_SWITCH_STEPS = (50, 150)                                    # :380-391 with sim_time = 1000
LANE_PATHS_OF = (0, 1, 0)

# mpc_kinematics.py:381-391, the weights and bounds INSIDE main's loop (QN's last entry is 50
# there, 100 before the loop, :353)
KINFROZEN_Q = np.diag([1.0, 1.0, 5.0, 10.0])
KINFROZEN_QN = np.diag([10.0, 10.0, 50.0, 50.0])
KINFROZEN_R = np.diag([0.1, 0.1])
KINFROZEN_UMIN = np.array([-np.deg2rad(15), -3.])
KINFROZEN_UMAX = np.array([np.deg2rad(15), 1.])
KINFROZEN_XMIN = np.array([-np.inf, -np.inf, -100., -np.pi])
KINFROZEN_XMAX = np.array([np.inf, np.inf, 100., np.pi])

# structural nonzeros of get_dynamics_model's Ad = I + dt Ac and Bd = dt Bc (vehicle_models.py:273-292)
DYN_MASK_A = np.eye(6, dtype=np.uint8)
for _i, _j in [(0, 2), (0, 3), (0, 4), (1, 2), (1, 3), (1, 4), (2, 5), (3, 3), (3, 4), (3, 5), (4, 3), (4, 4),
               (4, 5), (5, 3), (5, 4), (5, 5)]:
    DYN_MASK_A[_i, _j] = 1
DYN_MASK_B = np.zeros((6, 2), np.uint8)
DYN_MASK_B[3:, :] = 1


# --------------------------------------- path bank, lane-change loop, frozen-model loop --
def reference_search_paths(paths_x, paths_y, paths_yaw, path_id, set_speed, pred, dt):
    """mpc_device.hip::k_kin_reference_paths (mpcqp_kin_reference_search_paths_device) in numpy:
    reference_search / nearest_point of the kinematic scripts (reversed scan, strict <,
    look_ind 1) for B vehicles, vehicle b on path path_id[b] of the bank.

    paths_x, paths_y (npaths, npath); paths_yaw the same or None (yaw 0); path_id (B,) or None
    (path 0), clamped into [0, npaths); set_speed (B,); pred (B, N+1, nxa) stage-major with the
    speed in state 2 -> Xr (B, 4, N+1).  Where the reference would read past the path's end
    (IndexError) the index holds the start of the last segment."""
    paths_x, paths_y = np.atleast_2d(np.asarray(paths_x, float)), np.atleast_2d(np.asarray(paths_y, float))
    npaths, npt = paths_x.shape
    pred = np.asarray(pred, float)
    B, N1 = pred.shape[:2]
    pid = np.zeros(B, int) if path_id is None else np.clip(np.asarray(path_id), 0, npaths - 1)
    paths_yaw = np.zeros_like(paths_x) if paths_yaw is None else np.atleast_2d(np.asarray(paths_yaw, float))
    Xr = np.empty((B, 4, N1))
    for b in range(B):
        px, py = paths_x[pid[b]], paths_y[pid[b]]
        seg = lambda i: np.sqrt((px[i + 1] - px[i]) ** 2 + (py[i + 1] - py[i]) ** 2)
        min_d, ind = np.inf, -1
        for i in reversed(range(npt)):
            d = np.sqrt((px[i] - pred[b, 0, 0]) ** 2 + (py[i] - pred[b, 0, 1]) ** 2)
            if d < min_d:
                min_d, ind = d, i
        ind = min(ind + 1, npt - 2)
        path_d, cumul = seg(ind), 0.0
        for i in range(N1):
            cumul = cumul + abs(pred[b, i, 2]) * dt
            while cumul >= path_d and ind + 1 < npt - 1:
                ind += 1
                path_d = path_d + seg(ind)
            Xr[b, :, i] = px[ind], py[ind], set_speed[b], paths_yaw[pid[b], ind]
    return Xr


def lane_path_id(step, switch_steps=LANE_SWITCH_STEPS, paths_of=LANE_PATHS_OF):
    """The path loop pass `step` of mpc_increment_kinematics_pred_matrix.main searches (its two
    `if i > ...`, :380-391): paths_of[#{j : step > switch_steps[j]}], elementwise over step."""
    return slack_regime(step, switch_steps, paths_of)


def lane_tail(sol, Ad0, Bd0, gd0, xt, step, N, l_f, l_r, dt, switch_steps=LANE_SWITCH_STEPS,
              paths_of=LANE_PATHS_OF):
    """The tail of mpc_increment_kinematics_pred_matrix.main's loop (:423-472) for one vehicle,
    without its aliasing -- mpc_device.hip::k_lane_tail (mpcqp_lane_tail_device) in numpy.

    sol = (x~_0..x~_N, du_0..du_{N-1}); Ad0, Bd0, gd0 stage 0 of the linearisation; xt = x~ (6,)
    as the step started; step the number of steps taken so far.  Returns (row, xt, pred, pdu,
    step, path_id): row = x~ as the step started (plt_states, plt_actions: the input held BEFORE
    the step); xt = (Ad0 x + Bd0 u + gd0, u) with u = u_prev + du_0; pred (N+1, 6) = (xt,
    x~_2..x~_N, (update_kinematics_model(x_N, u_N), u_N)) -- the in-place shift makes the
    terminal control the solution's stage-N one; pdu (N+1, 2) = (du_1..du_{N-1}, du_{N-1},
    du_{N-1}); step + 1 and the path the next step searches."""
    sol, xt = np.asarray(sol, float), np.asarray(xt, float)
    S = sol[:(N + 1) * 6].reshape(N + 1, 6)
    D = sol[(N + 1) * 6:].reshape(N, 2)
    row = xt.copy()
    u = xt[4:] + D[0]
    xt = np.concatenate([(Ad0 @ xt[:4] + Bd0 @ u) + gd0, u])
    pred = np.empty((N + 1, 6)); pdu = np.empty((N + 1, 2))
    pred[0] = xt
    pred[1:N] = S[2:N + 1]
    pred[N] = np.concatenate([kin_update(l_f, l_r, dt, S[N, :4], S[N, 4:]), S[N, 4:]])
    pdu[0:N - 1] = D[1:N]
    pdu[N - 1] = pdu[N] = D[N - 1]
    step = int(step) + 1
    return row, xt, pred, pdu, step, int(lane_path_id(step, switch_steps, paths_of))


def kinfrozen_rollout(x0, pred_u0, N, l_f, l_r, dt):
    """Initial horizon of mpc_kinematics.main (:318-329) for one vehicle or a batch: x0 (.., 4);
    pred_u0 (.., N+1, 2) is the initial pred_u (the script's u0 + noise, last column repeated);
    pred_x (.., N+1, 4) has stage 0 = x0, stage i = update_kinematics_model(stage i-1,
    pred_u0[i]) for 1 <= i <= N-1 (the index is i, not i-1) and stage N = 0.  Returns (pred_x,
    x_start): the script rolls its own state forward in place (x0 IS x, :304), so its plant
    starts from x_start = pred_x[N-1], not x0."""
    x0, pred_u0 = np.asarray(x0, float), np.asarray(pred_u0, float)
    pred_x = np.zeros(x0.shape[:-1] + (N + 1, 4))
    pred_x[..., 0, :] = x0
    for i in range(1, N):
        pred_x[..., i, :] = kin_update(l_f, l_r, dt, pred_x[..., i - 1, :], pred_u0[..., i, :])
    return pred_x, pred_x[..., N - 1, :].copy()


def kinfrozen_tail(sol, status, Ad, Bd, gd, x, u, pred_x, N):
    """The tail of mpc_kinematics.main's loop (:397-456) for one vehicle --
    mpc_device.hip::k_kin_frozen_tail (mpcqp_kin_frozen_tail_device) in numpy.

    sol = (S_0..S_N, U_0..U_{N-1}); status the solver's code; Ad, Bd, gd the step's one model.
    Returns (row, x, u, pred_x, skipped).  A status other than 1 (`solved`) is the script's
    `continue`: (None, x, u, pred_x, True), everything as given.  Otherwise pred_x (N+1, 4) = the
    solution's states, stage 0 included, no shift; row = (x before the step, U_0); x = Ad x +
    Bd U_0 + gd; u = U_0."""
    if status != 1:
        return None, x, u, pred_x, True
    sol, x = np.asarray(sol, float), np.asarray(x, float)
    S = sol[:(N + 1) * 4].reshape(N + 1, 4)
    U0 = sol[(N + 1) * 4:(N + 1) * 4 + 2]
    row = np.concatenate([x, U0])
    return row, (Ad @ x + Bd @ U0) + gd, U0.copy(), S.copy(), False


def _lateral_x0(rng, B):
    return np.stack([rng.uniform(-.05, .05, B), rng.uniform(-.1, .1, B), rng.uniform(-10, 10, B) * DEG,
                     rng.uniform(-3, 3, B)], axis=1)


def make_batch(cfg: int, B: int | None = None, seed: int | None = None, N: int | None = None):
    """Synthetic batch for BASELINE.json config `cfg`.

    Returns dict(P, A: scipy CSC templates (shared pattern), Px (B,nnzP), Ax (B,nnzA),
    q (B,n), l (B,m), u (B,m), n, m, N, u_slice (slice of the first control in x),
    name, settings (the reference call site's osqp keywords))."""
    spec = CONFIGS[cfg]
    B = spec["B"] if B is None else B
    N = spec["N"] if N is None else N
    rng = np.random.default_rng(cfg if seed is None else seed)
    layout = spec["layout"]
    if layout == "vanilla":
        x0 = _lateral_x0(rng, B)
        P, q0, A, l0, u0 = vanilla_qp(LATERAL_AD, LATERAL_BD, np.zeros(4), np.zeros(4), np.zeros((4, N + 1)),
                                      VANILLA_Q, VANILLA_Q, VANILLA_R, N, VANILLA_XMIN, -VANILLA_XMIN,
                                      -VANILLA_UMAX, VANILLA_UMAX)
        nx, nu = 4, 1
        l = np.tile(l0, (B, 1)); u = np.tile(u0, (B, 1))
        l[:, :nx] = -x0; u[:, :nx] = -x0
        q = np.tile(q0, (B, 1))
        Px = np.tile(P.data, (B, 1)); Ax = np.tile(A.data, (B, 1))
        ucol = (N + 1) * nx
        settings = dict(verbose=False, warm_start=True)           # mpc_kinematics.py:195
        theta = np.concatenate([x0, np.zeros((B, 4 * (N + 1)))], axis=1)  # (x0, Xr): mpc_device.LateralAssembler
        regime = np.zeros(B, np.int32)
    elif layout == "slack":
        nx, nu = 5, 1
        x0 = np.concatenate([_lateral_x0(rng, B), rng.uniform(-5, 5, (B, 1)) * DEG], axis=1)
        P, q0, A, l0, u0 = slack_qp(N, np.zeros(nx))
        _, _, _, l1, _ = slack_qp(N, np.zeros(nx), regime=1)
        reg = rng.uniform(size=B) < 0.3                            # e_y >= 2 regime (:163-167)
        l = np.where(reg[:, None], l1[None], l0[None]).copy(); u = np.tile(u0, (B, 1))
        l[:, :nx] = -x0; u[:, :nx] = -x0
        q = np.tile(q0, (B, 1))
        Px = np.tile(P.data, (B, 1)); Ax = np.tile(A.data, (B, 1))
        ucol = (N + 1) * nx
        settings = dict(warm_start=True)                           # slack script :121
        theta = np.concatenate([x0, np.zeros((B, 4))], axis=1)     # (x~0, xr): mpc_device.LateralAssembler
        regime = reg.astype(np.int32)
    elif layout == "dynamic":
        veh = VehicleParams(dt=0.05)
        nx, nu = 6, 2
        xs = np.zeros((B, 6))
        xs[:, 2] = rng.uniform(-np.pi / 8, np.pi / 8, B)
        xs[:, 3] = rng.uniform(5, 25, B)
        xs[:, 4] = rng.uniform(-.5, .5, B)
        xs[:, 5] = rng.uniform(-.2, .2, B)
        us = np.stack([np.deg2rad(rng.uniform(-5, 5, B)), rng.uniform(-1, 1, B)], axis=1)
        yoff = rng.uniform(-4, 4, B)
        Ads, Bds, gds = [], [], []
        xk = xs.copy()
        for k in range(N):                                         # zero-increment rollout (:506-514)
            Ad, Bd, gd = linearise_dynamics(veh, xk, us)
            Ads.append(Ad); Bds.append(Bd); gds.append(gd)
            xk = np.einsum("bij,bj->bi", Ad, xk) + np.einsum("bij,bj->bi", Bd, us) + gd
        Ads = np.stack(Ads, 1); Bds = np.stack(Bds, 1); gds = np.stack(gds, 1)
        Xr = np.zeros((B, 6, N + 1))
        Xr[:, 0] = np.arange(N + 1)[None] * 10.0 * 0.05
        Xr[:, 1] = yoff[:, None]
        Xr[:, 3] = 10.0
        xt0 = np.concatenate([xs, us], axis=1)
        # shared pattern: every entry of Ad / Bd that is nonzero for some instance or stage
        maskA = np.abs(Ads).max(axis=(0, 1)) > 0
        maskB = np.abs(Bds).max(axis=(0, 1)) > 0
        P, _, A, _, _ = incremental_qp([np.where(maskA, 7.0, 0.0)] * N, [np.where(maskB, 7.0, 0.0)] * N,
                                       [np.zeros(6)] * N, np.zeros(8), np.zeros((6, N + 1)), DYN_Q, DYN_QN, DYN_R,
                                       N, DYN_XMIN_T, DYN_XMAX_T, DYN_DUMIN, -DYN_DUMIN)
        pa, pb, pb2 = _stage_positions(A, N, nx, nu, maskA, maskB)
        Ax = np.tile(A.data, (B, 1))
        ii, jj = np.nonzero(maskA)
        Ax[:, pa] = Ads[:, :, ii, jj].reshape(B, -1)
        ii2, jj2 = np.nonzero(maskB)
        Ax[:, pb] = Bds[:, :, ii2, jj2].reshape(B, -1)
        Ax[:, pb2] = Bds[:, :, ii2, jj2].reshape(B, -1)
        Px = np.tile(P.data, (B, 1))
        C = np.hstack([np.eye(nx), np.zeros((nx, nu))])
        qx = -np.einsum("ij,bjk->bki", (DYN_Q @ C).T, Xr[:, :, :N])
        qN = -np.einsum("ij,bj->bi", (DYN_QN @ C).T, Xr[:, :, N])
        q = np.concatenate([qx.reshape(B, -1), qN, np.zeros((B, N * nu))], axis=1)
        n_x = (N + 1) * (nx + nu)
        gt = np.concatenate([gds, np.zeros((B, N, nu))], axis=2).reshape(B, -1)
        leq = np.concatenate([-xt0, -gt], axis=1)
        lineq = np.concatenate([np.tile(DYN_XMIN_T, N + 1), np.tile(DYN_DUMIN, N)])
        uineq = np.concatenate([np.tile(DYN_XMAX_T, N + 1), np.tile(-DYN_DUMIN, N)])
        l = np.concatenate([leq, np.tile(lineq, (B, 1))], axis=1)
        u = np.concatenate([leq, np.tile(uineq, (B, 1))], axis=1)
        ucol = n_x
        settings = dict(verbose=True, polish=False, warm_start=False)   # mpc_dynamics.py:393
        theta = regime = None
    else:
        raise ValueError(layout)
    n, m = P.shape[0], A.shape[0]
    return dict(P=P, A=A, Px=np.ascontiguousarray(Px), Ax=np.ascontiguousarray(Ax), q=np.ascontiguousarray(q),
                l=np.ascontiguousarray(l), u=np.ascontiguousarray(u), n=n, m=m, N=N, B=B, nu=nu,
                u_slice=slice(ucol, ucol + nu), u_block=slice(ucol, ucol + N * nu), name=spec["name"],
                settings=settings, cfg=cfg, theta=theta, regime=regime)


def _stage_positions(A, N, nx, nu, maskA, maskB):
    """Indices into A.data of the Ad entries of A~_k, of the Bd entries of A~_k (u_prev
    columns) and of the Bd entries of B~_k (du_k columns), ordered (stage, mask nonzero)."""
    A = A.tocsc()
    nxa = nx + nu
    ncol_x = (N + 1) * nxa

    def pos(r, c):
        lo, hi = A.indptr[c], A.indptr[c + 1]
        k = lo + np.searchsorted(A.indices[lo:hi], r)
        assert k < hi and A.indices[k] == r, (r, c)
        return k

    ii, jj = np.nonzero(maskA)
    ii2, jj2 = np.nonzero(maskB)
    pa, pb = [], []
    for k in range(N):
        r0 = (k + 1) * nxa
        for i, j in zip(ii, jj):
            pa.append(pos(r0 + i, k * nxa + j))
        for i, j in zip(ii2, jj2):
            # Bd appears twice per stage: in A~ (column of u_prev) and in B~ (column of du_k).
            pb.append(pos(r0 + i, k * nxa + nx + j))
    pb2 = []
    for k in range(N):
        r0 = (k + 1) * nxa
        for i, j in zip(ii2, jj2):
            pb2.append(pos(r0 + i, ncol_x + k * nu + j))
    return np.array(pa), np.array(pb), np.array(pb2)
