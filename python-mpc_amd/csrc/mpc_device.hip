// mpc_device.hip -- the MPC data path around the solver, on the device
// (F1, the QP layouts and the assembly, is mpc_assembly.hip, F2, the
// linearisations, mpc_linearise.hip, the models themselves vehicle_model.h): the closed loops'
// own steps between two osqp solves of Control/MPC/mpc_dynamics.py:main, batched over B vehicles.
//
//   F3  k_reference<DynamicBicycle>   reference_search / nearest_point      mpc_dynamics.py:30-90
//       k_incr_shift                  plant step + horizon shift             mpc_dynamics.py:578-617
//                                     (terminal state: update_dynamics_model vehicle_models.py:343-477)
// and the same loop of Control/MPC/mpc_incre_kine_func.py:simulate on the kinematic bicycle:
//       k_reference<KinematicBicycle> reference_search / nearest_point        mpc_incre_kine_func.py:28-81
//       k_kin_shift                   record, stop rule, plant step, shift    mpc_incre_kine_func.py:382-428
// and the LTV MPC in the inputs themselves (mpcqp_ltv_layout: the same layout with nxa = nx), with
// the closed loop of Control/MPC/mpc_kinematics_pred_matrix.py:main:
//       k_kin_rollout                 initial horizon (nonlinear Euler)       :405-419
//       k_kin_ltv_shift               skip rule, record, plant step, shift    :479-563
// and the two remaining loops of Control/MPC: mpc_increment_kinematics_pred_matrix.py:main (the
// double lane change: a bank of paths, one selected per vehicle by a step schedule) and
// mpc_kinematics.py:main (one linearisation per step for every stage, no shift):
//       k_kin_reference_paths         reference_search on path_id[b] of a path bank   :41-83
//       k_lane_tail                   record, plant step, shift, path schedule        :380-391, :423-472
//       k_kin_frozen_tail             skip rule, unpack, record, plant step           mpc_kinematics.py:397-456
// and the one closed loop that keeps its problem alive, vehicle_lateral_mpc_slack_increment.py
// (setup once, update(q, l, u) + warm-started solve per step):
//       k_lti_step                    raise rule, record, plant step, schedule :158-172, :252-269
// The two bicycles are model structs (DynamicBicycle, KinematicBicycle) over which the
// reference walk is written once; the three shift kernels share the plant
// step, the trajectory append and kin_update, and keep their own shift and terminal-state rules.
//
// One thread per vehicle for the
// sequential parts (reference search walks the path, the shift reorders the
// horizon).  All fp64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../include/mpcqp.h"
#include "kernels.h"
#include "mpc_fleet.h"
#include "mpc_host.h"
#include "mpc_layout.h"
#include "vehicle_model.h"

namespace mpcqp {

// update_dynamics_model as the reference calls it: the low-speed guard on copies, then euler_step
__device__ void euler_step_guarded(const VehicleK& k, const double* xin, const double* uin, double* xn) {
    double x[6], u[2];
    for (int i = 0; i < 6; ++i) x[i] = xin[i];
    u[0] = uin[0]; u[1] = uin[1];
    low_speed_guard(x, u);
    euler_step<double>(k, x, u, xn);
}

// ---------------------------------------------------------- receding horizon --
// nearest_point (look_ind = 1) and the walk of reference_search along the path, as both
// scripts have them (mpc_dynamics.py:30-90, mpc_incre_kine_func.py:28-81): the path index
// steps forward while the travelled distance sum |v_i| dt exceeds the path length covered.
struct PathWalk {
    const double *px, *py;
    int np, ind;
    double path_d, cumul = 0.0;

    __device__ double seg(int i) const {
        return sqrt((px[i + 1] - px[i]) * (px[i + 1] - px[i]) + (py[i + 1] - py[i]) * (py[i + 1] - py[i]));
    }
    __device__ PathWalk(const double* px_, const double* py_, int np_, double X0, double Y0)
        : px(px_), py(py_), np(np_), ind(-1) {
        double min_d = INFINITY;
        for (int i = np - 1; i >= 0; --i) {  // reversed(range(len(path_x))), strict <
            const double d = sqrt((px[i] - X0) * (px[i] - X0) + (py[i] - Y0) * (py[i] - Y0));
            if (d < min_d) { min_d = d; ind = i; }
        }
        // look_ind = 1.  The reference reads path[ind + 1] from here on and raises
        // IndexError once ind reaches the last point; the walk holds the start of the
        // last segment (np - 2) instead.  A NaN position leaves ind = -1: 0 here (np >= 2).
        ind = min(ind + 1, np - 2);
        path_d = seg(ind);
    }
    // the path index after travelling at `speed` for dt more
    __device__ int advance(double speed, double dt) {
        cumul += fabs(speed) * dt;
        while (cumul >= path_d && ind + 1 < np - 1) {
            ind += 1;
            path_d += seg(ind);
        }
        return ind;
    }
};

// reference_search per vehicle: pred (B, N+1, nxa) stage-major with the speed in state
// M::SPEED;  Xr (B, M::NX, N+1), its columns by M::reference_column.
template <class M>
__global__ __launch_bounds__(128) void k_reference(long B, int N, int nxa, int np, const double* __restrict__ px,
                                                   const double* __restrict__ py, const double* __restrict__ pyaw,
                                                   const double* __restrict__ set_speed,
                                                   const double* __restrict__ pred, double dt,
                                                   double* __restrict__ Xr) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* pb = pred + b * (long)(N + 1) * nxa;
    PathWalk walk(px, py, np, pb[0], pb[1]);
    double* Xb = Xr + b * (long)M::NX * (N + 1);
    for (int i = 0; i <= N; ++i) {
        const int ind = walk.advance(pb[i * nxa + M::SPEED], dt);
        M::reference_column(Xb + i, N + 1, px[ind], py[ind], pyaw, ind, set_speed, b);
    }
}

// k_reference<KinematicBicycle> over a bank of `npaths` paths of np points each (path p at
// px / py / pyaw + p * np), vehicle b on path path_id[b] (null: path 0; clamped into the bank).
// pyaw null: yaw 0 on every point (reference_search of the two pred_matrix scripts and of
// mpc_kinematics.py, x_ref[3] = deg2rad(0)).
__global__ __launch_bounds__(128) void k_kin_reference_paths(long B, int N, int nxa, int npaths, int np,
                                                             const double* __restrict__ px,
                                                             const double* __restrict__ py,
                                                             const double* __restrict__ pyaw,
                                                             const int* __restrict__ path_id,
                                                             const double* __restrict__ set_speed,
                                                             const double* __restrict__ pred, double dt,
                                                             double* __restrict__ Xr) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int p = path_id ? min(max(path_id[b], 0), npaths - 1) : 0;
    const double* bx = px + (long)p * np;
    const double* by = py + (long)p * np;
    const double* pb = pred + b * (long)(N + 1) * nxa;
    PathWalk walk(bx, by, np, pb[0], pb[1]);
    double* Xb = Xr + b * (long)4 * (N + 1);
    for (int i = 0; i <= N; ++i) {
        const int ind = walk.advance(pb[i * nxa + KinematicBicycle::SPEED], dt);
        Xb[0 * (N + 1) + i] = bx[ind];
        Xb[1 * (N + 1) + i] = by[ind];
        Xb[2 * (N + 1) + i] = set_speed[b];
        Xb[3 * (N + 1) + i] = pyaw ? pyaw[(long)p * np + ind] : 0.0;
    }
}

// x_next = (A0 x + B0 u) + g0 of the linearised stage-0 model, in the reference's association.
// Inlined, so nx / nu are compile-time where the caller's are (the kinematic kernels) and run-time
// where they come from the layout (k_incr_shift; unrolled for nx = 6 the compiler orders the fma
// operands differently, and a state that is already NaN comes out with another NaN's sign).
__device__ __forceinline__ void plant_step(int nx, int nu, const double* A0, const double* B0, const double* g0,
                                           const double* x, const double* u, double* xnext) {
    for (int i = 0; i < nx; ++i) {
        double acc = 0.0;
        for (int j = 0; j < nx; ++j) acc += A0[i * nx + j] * x[j];
        double bu = 0.0;
        for (int j = 0; j < nu; ++j) bu += B0[i * nu + j] * u[j];
        xnext[i] = (acc + bu) + g0[i];
    }
}

// The next free row (`width` doubles) of vehicle b's trajectory record, counted in
// traj_len[b]; null when recording is off (traj_cap 0) or the record is full.
__device__ __forceinline__ double* traj_append(double* traj, int traj_cap, int* traj_len, long b, int width) {
    if (traj_cap <= 0) return nullptr;
    const int len = traj_len[b];
    if (len < 0 || len >= traj_cap) return nullptr;
    traj_len[b] = len + 1;
    return traj + (b * (long)traj_cap + len) * width;
}

// One-stage shift of a vector made of `groups` blocks of N+1 stages of width nxa followed
// by one block of N stages of width nu (x: groups 1, y: groups 2); element-parallel.
__global__ __launch_bounds__(256) void k_stage_shift(long total, int len, int N, int nxa, int nu, int groups,
                                                     const double* __restrict__ src, double* __restrict__ dst) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long b = e / len;
    const int i = (int)(e - b * len);
    const int stage_blk = (N + 1) * nxa, head = groups * stage_blk;
    int j;
    if (i < head) {
        const int g = i / stage_blk, r = i - g * stage_blk, k = r / nxa, c = r - k * nxa;
        j = g * stage_blk + min(k + 1, N) * nxa + c;
    } else {
        const int r = i - head, k = r / nu, c = r - k * nu;
        j = head + min(k + 1, N - 1) * nu + c;
    }
    dst[e] = src[b * len + j];
}

// plant step and horizon shift of mpc_dynamics.main (:578-617), per vehicle:
//   pred_x~[:, k] = sol[k nxa ..],  du[:, k] = sol[(N+1) nxa + k nu ..]  (mpc_increment :398-432)
//   u = u_past + du_0;  x_next = Ad_0 x + Bd_0 u + gd_0;  x~ = (x_next, u)
//   shift pred_x~ / du one stage; terminal state by one nonlinear Euler step from
//   (pred_x~[:nx, N], pred_x~[nx:, N-1]) (update_dynamics_model)
template <class KS>
__global__ __launch_bounds__(128) void k_incr_shift(KS ks, IncrK L, long B, const double* __restrict__ sol,
                                                    const double* __restrict__ Ad, const double* __restrict__ Bd,
                                                    const double* __restrict__ gd, double* __restrict__ xt,
                                                    double* __restrict__ pred, double* __restrict__ pdu) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int N = L.N, nx = L.nx, nu = L.nu, nxa = L.nxa, n = L.n;  // nx 6, nu 2: the entry point's check
    const double* s = sol + b * n;
    double* pb = pred + b * (long)(N + 1) * nxa;
    double* db = pdu + b * (long)(N + 1) * nu;
    double* xb = xt + b * nxa;
    // plant step (:581-586), stage 0 of the linearisation
    double xnext[8], uu[8];
    for (int j = 0; j < nu; ++j) uu[j] = xb[nx + j] + s[(N + 1) * nxa + j];
    plant_step(nx, nu, Ad + b * (long)N * nx * nx, Bd + b * (long)N * nx * nu, gd + b * (long)N * nx, xb, uu, xnext);
    for (int i = 0; i < nx; ++i) xb[i] = xnext[i];
    for (int j = 0; j < nu; ++j) xb[nx + j] = uu[j];
    // shift (:589-610) from the solution (the reference's temp copies are the solution)
    for (int i = 0; i < nxa; ++i) pb[i] = xb[i];
    for (int j = 0; j < nu; ++j) db[j] = s[(N + 1) * nxa + 1 * nu + j];
    for (int k = 1; k <= N - 2; ++k) {
        for (int i = 0; i < nxa; ++i) pb[k * nxa + i] = s[(k + 1) * nxa + i];
        for (int j = 0; j < nu; ++j) db[k * nu + j] = s[(N + 1) * nxa + (k + 1) * nu + j];
    }
    for (int i = 0; i < nxa; ++i) pb[(N - 1) * nxa + i] = s[N * nxa + i];
    for (int j = 0; j < nu; ++j) db[(N - 1) * nu + j] = s[(N + 1) * nxa + (N - 1) * nu + j];
    // terminal state (:604-608): Euler step of (x_N, u_{N-1}) of the solution
    double xN[6], uN[2], xe[6];
    for (int i = 0; i < 6; ++i) xN[i] = s[N * nxa + i];
    for (int j = 0; j < 2; ++j) uN[j] = s[(N - 1) * nxa + nx + j];
    euler_step_guarded(constants(ks, b), xN, uN, xe);
    for (int i = 0; i < nx; ++i) pb[N * nxa + i] = xe[i];
    for (int j = 0; j < nu; ++j) pb[N * nxa + nx + j] = pb[(N - 1) * nxa + nx + j];
    for (int j = 0; j < nu; ++j) db[N * nu + j] = db[(N - 1) * nu + j];
}

// VJP of euler_step_guarded, of the forward as it computes (k_linearise_vjp's rules): the guard
// first, then euler_step over duals in (yaw, vx, vy, r, steer, accel), seed 0 where the guard put a
// constant; w (6) the cotangent of the new state -> gx (6), gu (2).  X and Y pass with derivative 1.
__device__ void euler_step_vjp(const VehicleK& k, const double* xin, const double* uin, const double* w, double* gx,
                               double* gu) {
    double xg[6], ug[2];
    for (int i = 0; i < 6; ++i) xg[i] = xin[i];
    ug[0] = uin[0]; ug[1] = uin[1];
    const double vx_in = xg[3];
    low_speed_guard(xg, ug);
    const bool lat = !(vx_in > -0.5 && vx_in < 0.5), lon = !(vx_in > -0.3 && vx_in < 0.3);
    const Dual xd[6] = {Dual(xg[0]),          Dual(xg[1]),         Dual(xg[2], 0, true),
                        Dual(xg[3], 1, lon), Dual(xg[4], 2, lat), Dual(xg[5], 3, lat)};
    const Dual ud[2] = {Dual(ug[0], 4, lat), Dual(ug[1], 5, true)};
    Dual xe[6];
    euler_step<Dual>(k, xd, ud, xe);
    double g[Dual::ND];
    for (int q = 0; q < Dual::ND; ++q) g[q] = 0.0;
    for (int i = 0; i < 6; ++i)
        for (int q = 0; q < Dual::ND; ++q) g[q] += w[i] * xe[i].d[q];
    gx[0] = w[0];
    gx[1] = w[1];
    gx[2] = g[0];
    gx[3] = lon ? g[1] : 0.0;
    gx[4] = lat ? g[2] : 0.0;
    gx[5] = lat ? g[3] : 0.0;
    gu[0] = lat ? g[4] : 0.0;
    gu[1] = g[5];
}

// Plant step and in-place horizon shift that mpc_incre_kine_func.simulate (:385-387, :403-428) and
// mpc_increment_kinematics_pred_matrix.main (:442-472) share word for word, for one vehicle:
// s = (x~_0..x~_N, du_0..du_{N-1}) the solution, A0 / B0 / g0 stage 0 of the linearisation,
// xb = x~ (in/out), pb = pred_x~ (N+1 stages of 6), db = pred_du (N+1 stages of 2).
__device__ __forceinline__ void kin_incr_step_shift(const mpcqp_kin_vehicle& vk, int N, const double* s,
                                                    const double* A0, const double* B0, const double* g0,
                                                    double* xb, double* pb, double* db) {
    constexpr int nx = 4, nu = 2, nxa = 6;
    const double* D = s + (N + 1) * nxa;  // du_0 .. du_{N-1}
    // plant step, stage 0 of the linearisation
    double xnext[nx], uu[nu];
    for (int j = 0; j < nu; ++j) uu[j] = xb[nx + j] + D[j];
    plant_step(nx, nu, A0, B0, g0, xb, uu, xnext);
    for (int i = 0; i < nx; ++i) xb[i] = xnext[i];
    for (int j = 0; j < nu; ++j) xb[nx + j] = uu[j];
    // shift, from the solution
    for (int i = 0; i < nxa; ++i) pb[i] = xb[i];
    for (int k = 1; k <= N - 1; ++k)
        for (int i = 0; i < nxa; ++i) pb[k * nxa + i] = s[(k + 1) * nxa + i];
    for (int k = 0; k <= N - 2; ++k)
        for (int j = 0; j < nu; ++j) db[k * nu + j] = D[(k + 1) * nu + j];
    for (int j = 0; j < nu; ++j) db[(N - 1) * nu + j] = db[N * nu + j] = D[(N - 1) * nu + j];
    // terminal state: update_kinematics_model on (x_N, u_N) of the solution, v first
    const double* sN = s + N * nxa;
    kin_update(vk, sN, sN + nx, pb + N * nxa);
    for (int j = 0; j < nu; ++j) pb[N * nxa + nx + j] = sN[nx + j];
}

// Tail of mpc_incre_kine_func.simulate's loop (:382-428), per vehicle, in the reference's
// order: unpack the solution (mpc_increment :194-217), record the trajectory point
// (:389-393), stop rule (:395-401), plant step (:385-387, :403-405), horizon shift
// (:407-428).  The reference shifts pred_x~ in place (temp_pred_x_tilda IS pred_x_tilda),
// so by the time the terminal state is formed column N-1 already holds column N: the
// control of the terminal Euler step is the solution's stage-N control, not stage N-1's;
// update_kinematics_model (vehicle_models.py:877-880) then advances v before yaw uses it.
// A vehicle whose done flag is set is skipped whole.
template <class KS>
__global__ __launch_bounds__(128) void k_kin_shift(KS ks, IncrK L, long B, const double* __restrict__ sol,
                                                   const double* __restrict__ Ad, const double* __restrict__ Bd,
                                                   const double* __restrict__ gd, const double* __restrict__ Xr,
                                                   double* __restrict__ xt, double* __restrict__ pred,
                                                   double* __restrict__ pdu, int* __restrict__ finish_cnt,
                                                   int* __restrict__ done, double* __restrict__ traj, int traj_cap,
                                                   int* __restrict__ traj_len) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (done[b]) return;
    constexpr int nx = 4, nu = 2, nxa = 6;
    const int N = L.N, n = L.n;
    const double* s = sol + b * n;
    const double* D = s + (N + 1) * nxa;  // du_0 .. du_{N-1}
    double* pb = pred + b * (long)(N + 1) * nxa;
    double* db = pdu + b * (long)(N + 1) * nu;
    double* xb = xt + b * nxa;
    // trajectory point: the state the step started from and the first steer increment
    if (double* tr = traj_append(traj, traj_cap, traj_len, b, 4)) {
        tr[0] = xb[0]; tr[1] = xb[1]; tr[2] = xb[3]; tr[3] = D[0];
    }
    // stop rule: the reference breaks here, leaving pred_x~ / pred_du as mpc_increment unpacked them
    const double ex = Xr[b * (long)nx * (N + 1)] - xb[0], ey = Xr[b * (long)nx * (N + 1) + (N + 1)] - xb[1];
    if (sqrt(ex * ex + ey * ey) < 0.5) {
        const int c = finish_cnt[b] + 1;
        finish_cnt[b] = c;
        if (c > 15) {
            for (int i = 0; i < (N + 1) * nxa; ++i) pb[i] = s[i];
            for (int i = 0; i < N * nu; ++i) db[i] = D[i];
            for (int j = 0; j < nu; ++j) db[N * nu + j] = D[(N - 1) * nu + j];
            done[b] = 1;
            return;
        }
    }
    kin_incr_step_shift(constants(ks, b), N, s, Ad + b * (long)N * nx * nx, Bd + b * (long)N * nx * nu,
                        gd + b * (long)N * nx, xb, pb, db);
}

// A step schedule by value: value = val[#{j < nsw : step > sw[j]}] (k_lti_step's convention).
struct StepSchedule {
    int nsw;
    int sw[8], val[9];
    __device__ int at(int step) const {
        int r = 0;
        for (int j = 0; j < nsw; ++j) r += step > sw[j] ? 1 : 0;
        return val[r];
    }
};

// Tail of mpc_increment_kinematics_pred_matrix.main's loop (:423-472), per vehicle, in the
// reference's order: record plt_states / plt_actions (x~ as the step started: the input is the
// one held BEFORE the step), plant step and in-place shift (the text of simulate's, so
// kin_incr_step_shift), then the step counter and the path the NEXT step's reference search
// runs on (the double lane change of :380-391).  No skip rule: mpc_increment uses the solution
// whatever its status (:248-252).
template <class KS>
__global__ __launch_bounds__(128) void k_lane_tail(KS ks, IncrK L, StepSchedule sched, long B,
                                                   const double* __restrict__ sol, const double* __restrict__ Ad,
                                                   const double* __restrict__ Bd, const double* __restrict__ gd,
                                                   double* __restrict__ xt, double* __restrict__ pred,
                                                   double* __restrict__ pdu, int* __restrict__ step,
                                                   int* __restrict__ path_id, double* __restrict__ traj, int traj_cap,
                                                   int* __restrict__ traj_len) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    constexpr int nx = 4, nu = 2, nxa = 6;
    const int N = L.N;
    double* xb = xt + b * nxa;
    if (double* tr = traj_append(traj, traj_cap, traj_len, b, nxa))
        for (int i = 0; i < nxa; ++i) tr[i] = xb[i];
    kin_incr_step_shift(constants(ks, b), N, sol + b * L.n, Ad + b * (long)N * nx * nx, Bd + b * (long)N * nx * nu,
                        gd + b * (long)N * nx, xb, pred + b * (long)(N + 1) * nxa, pdu + b * (long)(N + 1) * nu);
    const int k = step[b] + 1;
    step[b] = k;
    path_id[b] = sched.at(k);
}

// Initial horizon of mpc_kinematics_pred_matrix.main (:405-419): u0 in every stage, the
// nonlinear model rolled forward from x0.  pred_x (B, N+1, 4), pred_u (B, N+1, 2).
template <class KS>
__global__ __launch_bounds__(128) void k_kin_rollout(KS ks, long B, int N, const double* __restrict__ x0,
                                                     const double* __restrict__ u0, double* __restrict__ pred_x,
                                                     double* __restrict__ pred_u) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const mpcqp_kin_vehicle& vk = constants(ks, b);
    double* px = pred_x + b * (long)(N + 1) * 4;
    double* pu = pred_u + b * (long)(N + 1) * 2;
    const double uu[2] = {u0[b * 2], u0[b * 2 + 1]};
    double xk[4];
    for (int i = 0; i < 4; ++i) xk[i] = px[i] = x0[b * 4 + i];
    for (int k = 0; k <= N; ++k) { pu[k * 2] = uu[0]; pu[k * 2 + 1] = uu[1]; }
    for (int k = 0; k < N; ++k) {
        kin_update(vk, xk, uu, xk);
        for (int i = 0; i < 4; ++i) px[(k + 1) * 4 + i] = xk[i];
    }
}

// Tail of mpc_kinematics_pred_matrix.main's loop (:479-563), per vehicle.  The reference
// shifts pred_x / pred_u in place through aliases; read from the solution (S_0..S_N,
// U_0..U_{N-1}) the result is: pred_x = (x_next, S_2..S_N, update(S_N, U_{N-1})),
// pred_u = (U_1..U_{N-1}, U_{N-1}, U_{N-1}) -- the terminal control is stage N-1, unlike
// k_kin_shift.  A vehicle whose status is not `solved` is skipped whole (:480-484).
template <class KS>
__global__ __launch_bounds__(128) void k_kin_ltv_shift(KS ks, int N, int n, long B, const double* __restrict__ sol,
                                                       const int* __restrict__ status, const double* __restrict__ Ad,
                                                       const double* __restrict__ Bd, const double* __restrict__ gd,
                                                       double* __restrict__ x, double* __restrict__ u,
                                                       double* __restrict__ pred_x, double* __restrict__ pred_u,
                                                       int* __restrict__ skipped, int* __restrict__ steps_taken,
                                                       double* __restrict__ traj, int traj_cap,
                                                       int* __restrict__ traj_len) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (status && status[b] != 1) {
        skipped[b] += 1;
        return;
    }
    constexpr int nx = 4, nu = 2;
    const double* S = sol + b * n;
    const double* U = S + (N + 1) * nx;
    double* xb = x + b * nx;
    double* ub = u + b * nu;
    double* px = pred_x + b * (long)(N + 1) * nx;
    double* pu = pred_u + b * (long)(N + 1) * nu;
    // plt_states[:, i], plt_actions[:, i]: the state the step started from, the control applied
    if (double* tr = traj_append(traj, traj_cap, traj_len, b, 6)) {
        for (int i = 0; i < nx; ++i) tr[i] = xb[i];
        tr[4] = U[0]; tr[5] = U[1];
    }
    // plant step (:534-541), stage 0 of the linearisation
    double xnext[nx];
    plant_step(nx, nu, Ad + b * (long)N * nx * nx, Bd + b * (long)N * nx * nu, gd + b * (long)N * nx, xb, U, xnext);
    for (int i = 0; i < nx; ++i) xb[i] = px[i] = xnext[i];
    for (int j = 0; j < nu; ++j) ub[j] = U[j];
    // shift (:543-563), from the solution
    for (int k = 1; k <= N - 1; ++k)
        for (int i = 0; i < nx; ++i) px[k * nx + i] = S[(k + 1) * nx + i];
    kin_update(constants(ks, b), S + N * nx, U + (N - 1) * nu, px + N * nx);
    for (int k = 0; k <= N - 2; ++k)
        for (int j = 0; j < nu; ++j) pu[k * nu + j] = U[(k + 1) * nu + j];
    for (int j = 0; j < nu; ++j) pu[(N - 1) * nu + j] = pu[N * nu + j] = U[(N - 1) * nu + j];
    if (steps_taken) steps_taken[b] += 1;
}

// The transposes of the differentiable loop tails as they compute, written once
// over a Tail.  One thread per (vehicle, output row), rows = the N+1 state rows of gsol (nxa wide),
// its N input rows (nu wide) and one row for the model and state outputs (gAd0, gBd0, ggd0, gxt):
// every output element has one writer, consecutive threads write consecutive rows of gsol, no
// atomics, and no thread walks the horizon.  (One thread per element would evaluate the terminal
// step's transpose nxa times per vehicle; this form does it in the one or two rows it lands in, and
// one thread per vehicle -- the forward's shape -- writes n strided doubles from one lane.)
// sol = (x~_0..x~_N, v_0..v_{N-1}), x~ the state (augmented by the applied input where the loop is
// incremental) and v the loop's input variable; xt the value from BEFORE the step.  Cotangents gxt
// (B,nxa), gu (B,nu; direct input only), gpred (B,N+1,nxa), gpdu (B,N+1,nu) of the NEW xt, u, pred,
// pdu, each null = zero; every output may be null.  With w = gxt + gpred[0], mode 0:
//   plant step   gAd0 = w_x x',  gBd0 = w_x u',  ggd0 = w_x,  gxt = Ad0' w_x (state part);
//                incremental (u = u_prev + v_0):  g u = w_u + Bd0' w_x,  gxt's input part = g v_0 = g u
//                direct (u = v_0; the old u is not read by the forward):  g v_0 = Bd0' w_x + gu
//   shift        g x~_k = gpred[k-1] (2 <= k <= N),  g v_k = gpdu[k-1] (1 <= k <= N-1);  v_{N-1} also
//                takes gpdu[N-1] and gpdu[N], added in that order; incremental: pred[N]'s input part is
//                x~_N's, which takes gpred[N]'s
//   terminal     Tail::terminal, the transpose of the step that formed pred[N]'s state part, added
//                last into the rows it touches
// mode (null = 0 everywhere; a Tail with modes = 1 has none) says what the forward did with the
// vehicle: 0 stepped; 1 left untouched (done was set / status != solved): gsol and the model outputs
// are zero and the state's cotangent passes through; 2 (modes = 3 only) met the stop rule on this
// step: pred / pdu took the unpacked solution (g x~_k = gpred[k], g v_k = gpdu[k], v_{N-1} also
// gpdu[N]), xt did not move.  The cotangent of the PREVIOUS horizon (gpred / gpdu in mode 1, zero
// otherwise) is the caller's to form.
//
// A Tail states the widths, whether the input is incremental, how many modes it knows, and
// terminal(vk, N, s, wN, row, g): wN = gpred[N], g the cotangent of output row `row` of gsol
// (row <= N: x~_row, else v_{row-N-1}).

// k_incr_shift: pred[N] = (euler_step_guarded(x_N, u_{N-1}), u_N): euler_step_vjp into x~_N's
// states and x~_{N-1}'s inputs.  The dual Euler step runs twice per vehicle, in rows N-1 and N.
struct DynamicIncrTail {
    using K = VehicleK;
    static constexpr int nx = 6, nu = 2, nxa = 8, modes = 1;
    static constexpr bool incremental = true;
    static constexpr const char* model = "6-state dynamic";
    static __device__ void terminal(const K& vk, int N, const double* s, const double* wN, int row, double* g) {
        if (row != N && row != N - 1) return;
        double ge[nx], gue[nu];
        euler_step_vjp(vk, s + N * nxa, s + (N - 1) * nxa + nx, wN, ge, gue);
        if (row == N)
            for (int i = 0; i < nx; ++i) g[i] = g[i] + ge[i];
        if (row == N - 1)
            for (int j = 0; j < nu; ++j) g[nx + j] = g[nx + j] + gue[j];
    }
};

// k_kin_shift / k_lane_tail (kin_incr_step_shift): pred[N] = (kin_update(x_N, u_N), u_N):
// kin_update_vjp into x~_N in both its parts, the input part after gpred[N]'s.
struct KinIncrTail {
    using K = mpcqp_kin_vehicle;
    static constexpr int nx = 4, nu = 2, nxa = 6, modes = 3;
    static constexpr bool incremental = true;
    static constexpr const char* model = "4-state kinematic";
    static __device__ void terminal(const K& vk, int N, const double* s, const double* wN, int row, double* g) {
        if (row != N) return;
        double ge[nx], gue[nu];
        kin_update_vjp(vk, s + N * nxa, s + N * nxa + nx, wN, ge, gue);
        for (int i = 0; i < nx; ++i) g[i] = g[i] + ge[i];
        for (int j = 0; j < nu; ++j) g[nx + j] = g[nx + j] + gue[j];
    }
};

// k_kin_ltv_shift's executed branch, sol = (S_0..S_N, U_0..U_{N-1}): pred_x[N] = kin_update(S_N,
// U_{N-1}): kin_update_vjp into S_N and into U_{N-1} (at N = 2 that is U_1, which takes the shift's
// triple sum and this at once).
struct KinLtvTail {
    using K = mpcqp_kin_vehicle;
    static constexpr int nx = 4, nu = 2, nxa = 4, modes = 2;
    static constexpr bool incremental = false;
    static constexpr const char* model = "4-state kinematic";
    static __device__ void terminal(const K& vk, int N, const double* s, const double* wN, int row, double* g) {
        if (row != N && row != 2 * N) return;
        double ge[nx], gue[nu];
        kin_update_vjp(vk, s + N * nx, s + (N + 1) * nx + (N - 1) * nu, wN, ge, gue);
        if (row == N)
            for (int i = 0; i < nx; ++i) g[i] = g[i] + ge[i];
        else
            for (int j = 0; j < nu; ++j) g[j] = g[j] + gue[j];
    }
};

template <class Tail>
__global__ __launch_bounds__(256) void k_tail_vjp(typename Tail::K vk, int N, int n, long B,
                                                  const double* __restrict__ sol, const double* __restrict__ Ad,
                                                  const double* __restrict__ Bd, const double* __restrict__ xt,
                                                  const int* __restrict__ dmode, const double* __restrict__ gxt,
                                                  const double* __restrict__ gu, const double* __restrict__ gpred,
                                                  const double* __restrict__ gpdu, double* __restrict__ gsol,
                                                  double* __restrict__ gAd0, double* __restrict__ gBd0,
                                                  double* __restrict__ ggd0, double* __restrict__ gxt_o) {
    constexpr int nx = Tail::nx, nu = Tail::nu, nxa = Tail::nxa;  // the entry point's check
    constexpr bool stops = Tail::modes == 3;
    const int rows = 2 * N + 2;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * rows) return;
    const long b = t / rows;
    const int row = (int)(t - b * rows);
    const int mode = (Tail::modes > 1 && dmode) ? dmode[b] : 0;
    const double* s = sol + b * n;
    const double* gp = gpred ? gpred + b * (long)(N + 1) * nxa : nullptr;
    const double* gd = gpdu ? gpdu + b * (long)(N + 1) * nu : nullptr;
    if (row <= N) {  // g x~_row
        if (!gsol) return;
        const int k = row;
        double g[nxa];
        if (mode != 0) {
            for (int i = 0; i < nxa; ++i) g[i] = (stops && mode == 2 && gp) ? gp[k * nxa + i] : 0.0;
        } else {
            for (int i = 0; i < nxa; ++i) g[i] = (k >= 2 && gp) ? gp[(k - 1) * nxa + i] : 0.0;
            if constexpr (Tail::incremental)
                if (k == N && gp)
                    for (int j = 0; j < nu; ++j) g[nx + j] = g[nx + j] + gp[N * nxa + nx + j];
            if (gp) Tail::terminal(constants(vk, b), N, s, gp + N * nxa, row, g);
        }
        for (int i = 0; i < nxa; ++i) gsol[b * n + k * nxa + i] = g[i];
        return;
    }
    if constexpr (Tail::modes > 1)
        if (mode != 0) {  // nothing went through the plant step
            if (row <= 2 * N) {
                if (!gsol) return;
                const int k = row - (N + 1);
                for (int j = 0; j < nu; ++j) {
                    double g = (stops && mode == 2 && gd) ? gd[k * nu + j] : 0.0;
                    if (stops && mode == 2 && gd && k == N - 1) g = g + gd[N * nu + j];
                    gsol[b * n + (N + 1) * nxa + k * nu + j] = g;
                }
                return;
            }
            for (int i = 0; i < nx; ++i) {
                if (gAd0)
                    for (int j = 0; j < nx; ++j) gAd0[b * nx * nx + i * nx + j] = 0.0;
                if (gBd0)
                    for (int j = 0; j < nu; ++j) gBd0[b * nx * nu + i * nu + j] = 0.0;
                if (ggd0) ggd0[b * nx + i] = 0.0;
            }
            if (gxt_o)
                for (int i = 0; i < nxa; ++i) gxt_o[b * nxa + i] = gxt ? gxt[b * nxa + i] : 0.0;
            return;
        }
    // w, the cotangent of the stepped x~, and that of the first input: what the rows below share
    const double* B0 = Bd + b * (long)N * nx * nu;
    double w[nxa], gv0[nu];
    for (int i = 0; i < nxa; ++i) w[i] = (gxt ? gxt[b * nxa + i] : 0.0) + (gp ? gp[i] : 0.0);
    const auto first_input = [&](int j) {  // g v_0
        double acc = 0.0;
        for (int i = 0; i < nx; ++i) acc += B0[i * nu + j] * w[i];
        if constexpr (Tail::incremental) return w[nx + j] + acc;
        else return acc + (gu ? gu[b * nu + j] : 0.0);
    };
    // incremental: input row 0 and the model row read it, and forming it in every row measured
    // faster than doing so under their branches; direct: input row 0 alone forms it
    if constexpr (Tail::incremental)
        for (int j = 0; j < nu; ++j) gv0[j] = first_input(j);
    if (row <= 2 * N) {  // g v_k
        if (!gsol) return;
        const int k = row - (N + 1);
        double g[nu];
        for (int j = 0; j < nu; ++j) {
            if (k == 0) g[j] = Tail::incremental ? gv0[j] : first_input(j);
            else g[j] = gd ? gd[(k - 1) * nu + j] : 0.0;
            if (k == N - 1 && gd) g[j] = (g[j] + gd[(N - 1) * nu + j]) + gd[N * nu + j];
        }
        if (gp) Tail::terminal(constants(vk, b), N, s, gp + N * nxa, row, g);
        for (int j = 0; j < nu; ++j) gsol[b * n + (N + 1) * nxa + k * nu + j] = g[j];
        return;
    }
    // the model row
    const double* A0 = Ad + b * (long)N * nx * nx;
    const double* xb = xt + b * nxa;
    double uu[nu];
    for (int j = 0; j < nu; ++j)
        uu[j] = Tail::incremental ? xb[nx + j] + s[(N + 1) * nxa + j] : s[(N + 1) * nxa + j];
    for (int i = 0; i < nx; ++i) {
        if (gAd0)
            for (int j = 0; j < nx; ++j) gAd0[b * nx * nx + i * nx + j] = w[i] * xb[j];
        if (gBd0)
            for (int j = 0; j < nu; ++j) gBd0[b * nx * nu + i * nu + j] = w[i] * uu[j];
        if (ggd0) ggd0[b * nx + i] = w[i];
    }
    if (gxt_o) {
        for (int j = 0; j < nx; ++j) {
            double acc = 0.0;
            for (int i = 0; i < nx; ++i) acc += A0[i * nx + j] * w[i];
            gxt_o[b * nxa + j] = acc;
        }
        if constexpr (Tail::incremental)
            for (int j = 0; j < nu; ++j) gxt_o[b * nxa + nx + j] = gv0[j];
    }
}


// Tail of mpc_kinematics.main's loop (:397-456), per vehicle.  One model (the linearisation at
// the current (x, u)) serves every stage, so Ad / Bd / gd are read at stage 0 of the (B, N, ..)
// lists the assembly took.  A vehicle whose status is not `solved` is skipped whole (:398-402).
// Otherwise pred_x takes the solution's states S_0..S_N with no shift -- stage 0 is S_0, not the
// plant state (:410-420) -- the record is (x before the step, U_0) (:452-453), and the plant
// steps with that same linear model (:449-455).
__global__ __launch_bounds__(128) void k_kin_frozen_tail(int N, int n, long B, const double* __restrict__ sol,
                                                         const int* __restrict__ status,
                                                         const double* __restrict__ Ad, const double* __restrict__ Bd,
                                                         const double* __restrict__ gd, double* __restrict__ x,
                                                         double* __restrict__ u, double* __restrict__ pred_x,
                                                         int* __restrict__ skipped, int* __restrict__ steps_taken,
                                                         double* __restrict__ traj, int traj_cap,
                                                         int* __restrict__ traj_len) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (status && status[b] != MPCQP_SOLVED) {
        skipped[b] += 1;
        return;
    }
    constexpr int nx = 4, nu = 2;
    const double* S = sol + b * n;
    const double* U = S + (N + 1) * nx;
    double* xb = x + b * nx;
    double* px = pred_x + b * (long)(N + 1) * nx;
    for (int i = 0; i < (N + 1) * nx; ++i) px[i] = S[i];
    if (double* tr = traj_append(traj, traj_cap, traj_len, b, 6)) {
        for (int i = 0; i < nx; ++i) tr[i] = xb[i];
        tr[4] = U[0]; tr[5] = U[1];
    }
    double xnext[nx];
    plant_step(nx, nu, Ad + b * (long)N * nx * nx, Bd + b * (long)N * nx * nu, gd + b * (long)N * nx, xb, U, xnext);
    for (int i = 0; i < nx; ++i) xb[i] = xnext[i];
    for (int j = 0; j < nu; ++j) u[b * nu + j] = U[j];
    if (steps_taken) steps_taken[b] += 1;
}

// ---- the LTI closed loop that keeps one problem alive (vehicle_lateral_mpc_slack_increment.py) ----
// The model x~+ = At x~ + Bt du and the step schedule of the bound regimes, by value.
struct LtiK {
    int nxa, nu, n, du_off, slack_off, nsw;
    int sw[8], reg[9];          // regime = reg[#{j < nsw : step > sw[j]}]
    double At[64], Bt[16];      // row-major nxa x nxa, nxa x nu
};

// x+ = At x + Bt du with every product and every sum rounded on its own, in this order, so that
// osqp_amd.mpc.lti_step reproduces it bit for bit in numpy: per row acc = At[i][0] x[0], then
// + At[i][j] x[j] for j = 1.., bu = Bt[i][0] du[0] (+ Bt[i][1] du[1]), x+[i] = acc + bu.
__device__ __forceinline__ void lti_plant_step(const LtiK& K, const double* x, const double* du, double* xnext) {
#pragma clang fp contract(off)
    const int nxa = K.nxa, nu = K.nu;
    for (int i = 0; i < nxa; ++i) {
        double acc = K.At[i * nxa] * x[0];
        for (int j = 1; j < nxa; ++j) acc = acc + K.At[i * nxa + j] * x[j];
        double bu = K.Bt[i * nu] * du[0];
        for (int j = 1; j < nu; ++j) bu = bu + K.Bt[i * nu + j] * du[j];
        xnext[i] = acc + bu;
    }
}

// Tail of the slack script's loop (:252-269), per vehicle: the `raise` on a solve that did not
// end `solved` (the vehicle is frozen: failed, fail_step), the record (plt_x_1..4, plt_u,
// plt_del_u, plt_s: the states the step started from, the control after it, du_0, the slack),
// the plant step, and the step counter with the bound regime the NEXT step assembles with
// (:158-172).  xt: x~ of vehicle b at xt[b * xt_stride], in/out.
__global__ __launch_bounds__(128) void k_lti_step(LtiK K, long B, const double* __restrict__ sol,
                                                  const int* __restrict__ status, double* __restrict__ xt,
                                                  long xt_stride, int* __restrict__ step, int* __restrict__ regime,
                                                  int* __restrict__ failed, int* __restrict__ fail_step,
                                                  double* __restrict__ traj, int traj_cap,
                                                  int* __restrict__ traj_len) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (failed[b]) return;
    if (status[b] != MPCQP_SOLVED) {
        failed[b] = 1;
        fail_step[b] = step[b];
        return;
    }
    const int nxa = K.nxa, nu = K.nu;
    const double* s = sol + b * K.n;
    double* xb = xt + b * xt_stride;
    double x[8], xnext[8], du[2];
    for (int i = 0; i < nxa; ++i) x[i] = xb[i];
    for (int j = 0; j < nu; ++j) du[j] = s[K.du_off + j];
    lti_plant_step(K, x, du, xnext);
    if (double* tr = traj_append(traj, traj_cap, traj_len, b, nxa + nu + 1)) {
        for (int i = 0; i < nxa - nu; ++i) tr[i] = x[i];
        for (int i = nxa - nu; i < nxa; ++i) tr[i] = xnext[i];
        for (int j = 0; j < nu; ++j) tr[nxa + j] = du[j];
        tr[nxa + nu] = K.slack_off >= 0 ? s[K.slack_off] : 0.0;
    }
    for (int i = 0; i < nxa; ++i) xb[i] = xnext[i];
    const int k = step[b] + 1;
    step[b] = k;
    int r = 0;
    for (int j = 0; j < K.nsw; ++j) r += k > K.sw[j] ? 1 : 0;
    regime[b] = K.reg[r];
}

}  // namespace mpcqp

using namespace mpcqp;

namespace {

template <class V>
int incr_shift_device(const mpcqp_incr_layout* L, const V* veh, int64_t B, const double* dsol, const double* dAd,
                      const double* dBd, const double* dgd, double* dxt, double* dpred, double* dpdu, void* stream) {
    if (!L || !veh || !dsol || !dAd || !dBd || !dgd || !dxt || !dpred || !dpdu || B < 0)
        return set_error(MPCQP_EINVAL, "incr_shift: bad arguments");
    if (L->nx != 6 || L->nu != 2)
        return set_error(MPCQP_EUNSUPPORTED, "incr_shift: the plant model is the 6-state dynamic bicycle (nx 6, nu 2)");
    if (int e = source_check("incr_shift", veh, B, L->dev)) return e;
    if (B == 0) return 0;
    if (int e = ensure_device(*const_cast<mpcqp_incr_layout*>(L))) return e;
    return launch_from(veh, L->dev, stream, B, 128, BOTH_FORMS(k_incr_shift, VehicleK), incr_k(*L), B, dsol, dAd, dBd,
                       dgd, dxt, dpred, dpdu);
}

template <class V>
int kin_shift_device(const mpcqp_incr_layout* L, const V* veh, int64_t B, const double* dsol, const double* dAd,
                     const double* dBd, const double* dgd, const double* dXr, double* dxt, double* dpred,
                     double* dpdu, int32_t* dfinish_cnt, int32_t* ddone, double* dtraj, int32_t traj_cap,
                     int32_t* dtraj_len, void* stream) {
    if (!L || !veh || !dsol || !dAd || !dBd || !dgd || !dXr || !dxt || !dpred || !dpdu || !dfinish_cnt || !ddone ||
        B < 0 || traj_cap < 0 || (traj_cap > 0 && (!dtraj || !dtraj_len)))
        return set_error(MPCQP_EINVAL, "kin_shift: bad arguments");
    if (L->nx != 4 || L->nu != 2)
        return set_error(MPCQP_EUNSUPPORTED, "kin_shift: the plant model is the 4-state kinematic bicycle (nx 4, nu 2)");
    if (int e = source_check("kin_shift", veh, B, L->dev)) return e;
    if (B == 0) return 0;
    if (int e = ensure_device(*const_cast<mpcqp_incr_layout*>(L))) return e;
    return launch_from(veh, L->dev, stream, B, 128, BOTH_FORMS(k_kin_shift, mpcqp_kin_vehicle), incr_k(*L), B, dsol, dAd, dBd, dgd,
                       dXr, dxt, dpred, dpdu, dfinish_cnt, ddone, dtraj, traj_cap, dtraj_len);
}

template <class V>
int kin_rollout_device(const V* veh, int64_t B, int32_t N, const double* dx0, const double* du0, double* dpred_x,
                       double* dpred_u, int32_t device, void* stream) {
    if (!veh || !dx0 || !du0 || !dpred_x || !dpred_u || B < 0 || N < 1)
        return set_error(MPCQP_EINVAL, "kin_rollout: bad arguments");
    if (int e = source_check("kin_rollout", veh, B, device)) return e;
    if (B == 0) return 0;
    return launch_from(veh, device, stream, B, 128, BOTH_FORMS(k_kin_rollout, mpcqp_kin_vehicle), B, N, dx0, du0, dpred_x,
                       dpred_u);
}

template <class V>
int kin_ltv_shift_device(const mpcqp_ltv_layout* L, const V* veh, int64_t B, const double* dsol,
                         const int32_t* dstatus, const double* dAd, const double* dBd, const double* dgd, double* dx,
                         double* du, double* dpred_x, double* dpred_u, int32_t* dskipped, int32_t* dsteps_taken,
                         double* dtraj, int32_t traj_cap, int32_t* dtraj_len, void* stream) {
    if (!L || !veh || !dsol || !dAd || !dBd || !dgd || !dx || !du || !dpred_x || !dpred_u || !dskipped || B < 0 ||
        traj_cap < 0 || (traj_cap > 0 && (!dtraj || !dtraj_len)))
        return set_error(MPCQP_EINVAL, "kin_ltv_shift: bad arguments");
    if (L->nx != 4 || L->nu != 2)
        return set_error(MPCQP_EUNSUPPORTED,
                         "kin_ltv_shift: the plant model is the 4-state kinematic bicycle (nx 4, nu 2)");
    if (int e = source_check("kin_ltv_shift", veh, B, L->dev)) return e;
    if (B == 0) return 0;
    return launch_from(veh, L->dev, stream, B, 128, BOTH_FORMS(k_kin_ltv_shift, mpcqp_kin_vehicle), L->N, L->n, B, dsol,
                       dstatus, dAd, dBd, dgd, dx, du, dpred_x, dpred_u, dskipped, dsteps_taken, dtraj, traj_cap,
                       dtraj_len);
}

template <class V>
int lane_tail_device(const mpcqp_incr_layout* L, const V* veh, int64_t B, const double* dsol, const double* dAd,
                     const double* dBd, const double* dgd, double* dxt, double* dpred, double* dpdu, int32_t nsw,
                     const int32_t* switch_steps, const int32_t* paths_of, int32_t* dstep, int32_t* dpath_id,
                     double* dtraj, int32_t traj_cap, int32_t* dtraj_len, void* stream) {
    if (nsw > 8) return set_error(MPCQP_EUNSUPPORTED, "lane_tail: need nsw <= 8");
    if (!L || !veh || !dsol || !dAd || !dBd || !dgd || !dxt || !dpred || !dpdu || !paths_of || !dstep || !dpath_id ||
        B < 0 || nsw < 0 || (nsw > 0 && !switch_steps) || traj_cap < 0 || (traj_cap > 0 && (!dtraj || !dtraj_len)))
        return set_error(MPCQP_EINVAL, "lane_tail: bad arguments");
    if (L->nx != 4 || L->nu != 2)
        return set_error(MPCQP_EUNSUPPORTED,
                         "lane_tail: the plant model is the 4-state kinematic bicycle (nx 4, nu 2)");
    if (int e = source_check("lane_tail", veh, B, L->dev)) return e;
    if (B == 0) return 0;
    if (int e = ensure_device(*const_cast<mpcqp_incr_layout*>(L))) return e;
    StepSchedule sched = {};
    sched.nsw = nsw;
    std::copy(switch_steps, switch_steps + nsw, sched.sw);
    std::copy(paths_of, paths_of + nsw + 1, sched.val);
    return launch_from(veh, L->dev, stream, B, 128, BOTH_FORMS(k_lane_tail, mpcqp_kin_vehicle), incr_k(*L), sched, B, dsol, dAd,
                       dBd, dgd, dxt, dpred, dpdu, dstep, dpath_id, dtraj, traj_cap, dtraj_len);
}

// dmode: null where the Tail has no modes; dgu: the direct-input Tail's, else null.  Every
// cotangent and every output may be null.
template <class Tail, class V>
int tail_vjp_device(const char* what, const IncrLayout* L, const V* veh, int64_t B, const double* dsol,
                    const double* dAd, const double* dBd, const double* dx_before, const int32_t* dmode,
                    const double* dgx, const double* dgu, const double* dgpred, const double* dgpdu, double* dgsol,
                    double* dgAd0, double* dgBd0, double* dggd0, double* dgx_before, void* stream) {
    if (!L || !veh || !dsol || !dAd || !dBd || !dx_before || B < 0)
        return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (L->nx != Tail::nx || L->nu != Tail::nu)
        return set_error(MPCQP_EUNSUPPORTED, "%s: the plant model is the %s bicycle (nx %d, nu %d)", what, Tail::model,
                         Tail::nx, Tail::nu);
    if (int e = source_check(what, veh, B, L->dev)) return e;
    if (B == 0 || (!dgsol && !dgAd0 && !dgBd0 && !dggd0 && !dgx_before)) return 0;
    return launch_from(veh, L->dev, stream, B * (2 * L->N + 2), 256, k_tail_vjp<Tail>, k_tail_vjp<OverFleet<Tail>>,
                       L->N, L->n, B, dsol, dAd, dBd, dx_before, dmode, dgx, dgu, dgpred, dgpdu, dgsol, dgAd0, dgBd0,
                       dggd0, dgx_before);
}

// dpath_yaw, dset_speed: the kinematic reference's (its entry point checks them), else null
template <class M>
int reference_device(const char* what, int64_t B, int32_t N, int32_t nxa, int32_t npath, const double* dpath_x,
                     const double* dpath_y, const double* dpath_yaw, const double* dset_speed, const double* dpred,
                     double dt, double* dXr, int32_t device, void* stream) {
    if (!dpath_x || !dpath_y || !dpred || !dXr || B < 0 || N < 1 || nxa < 4 || npath < 2)
        return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (B == 0) return 0;
    return launch(device, stream, B, 128, k_reference<M>, B, N, nxa, npath, dpath_x, dpath_y, dpath_yaw, dset_speed,
                  dpred, dt, dXr);
}

}  // namespace

extern "C" {

int mpcqp_reference_search_device(int64_t B, int32_t N, int32_t nxa, int32_t npath, const double* dpath_x,
                                  const double* dpath_y, const double* dpred, double dt, double* dXr, int32_t device,
                                  void* stream) {
    return reference_device<DynamicBicycle>("reference_search", B, N, nxa, npath, dpath_x, dpath_y, nullptr, nullptr,
                                            dpred, dt, dXr, device, stream);
}

int mpcqp_kin_reference_search_device(int64_t B, int32_t N, int32_t nxa, int32_t npath, const double* dpath_x,
                                      const double* dpath_y, const double* dpath_yaw, const double* dset_speed,
                                      const double* dpred, double dt, double* dXr, int32_t device, void* stream) {
    if (!dpath_yaw || !dset_speed) return set_error(MPCQP_EINVAL, "kin_reference_search: bad arguments");
    return reference_device<KinematicBicycle>("kin_reference_search", B, N, nxa, npath, dpath_x, dpath_y, dpath_yaw,
                                              dset_speed, dpred, dt, dXr, device, stream);
}

int mpcqp_incr_shift_device(const mpcqp_incr_layout* L, const mpcqp_vehicle* veh, int64_t B, const double* dsol,
                            const double* dAd, const double* dBd, const double* dgd, double* dxt, double* dpred,
                            double* dpdu, void* stream) {
    return incr_shift_device(L, veh, B, dsol, dAd, dBd, dgd, dxt, dpred, dpdu, stream);
}

int mpcqp_incr_shift_vjp_device(const mpcqp_incr_layout* L, const mpcqp_vehicle* veh, int64_t B, const double* dsol,
                                const double* dAd, const double* dBd, const double* dgd, const double* dxt_before,
                                const double* dgxt, const double* dgpred, const double* dgpdu, double* dgsol,
                                double* dgAd0, double* dgBd0, double* dggd0, double* dgxt_before, void* stream) {
    (void)dgd;  // the step is affine in gd: its VJP does not read it
    return tail_vjp_device<DynamicIncrTail>("incr_shift_vjp", L, veh, B, dsol, dAd, dBd, dxt_before, nullptr, dgxt,
                                            nullptr, dgpred, dgpdu, dgsol, dgAd0, dgBd0, dggd0, dgxt_before, stream);
}

int mpcqp_kin_shift_device(const mpcqp_incr_layout* L, const mpcqp_kin_vehicle* veh, int64_t B, const double* dsol,
                           const double* dAd, const double* dBd, const double* dgd, const double* dXr, double* dxt,
                           double* dpred, double* dpdu, int32_t* dfinish_cnt, int32_t* ddone, double* dtraj,
                           int32_t traj_cap, int32_t* dtraj_len, void* stream) {
    return kin_shift_device(L, veh, B, dsol, dAd, dBd, dgd, dXr, dxt, dpred, dpdu, dfinish_cnt, ddone, dtraj, traj_cap,
                            dtraj_len, stream);
}

int mpcqp_kin_rollout_device(const mpcqp_kin_vehicle* veh, int64_t B, int32_t N, const double* dx0,
                             const double* du0, double* dpred_x, double* dpred_u, int32_t device, void* stream) {
    return kin_rollout_device(veh, B, N, dx0, du0, dpred_x, dpred_u, device, stream);
}

int mpcqp_kin_ltv_shift_device(const mpcqp_ltv_layout* L, const mpcqp_kin_vehicle* veh, int64_t B,
                               const double* dsol, const int32_t* dstatus, const double* dAd, const double* dBd,
                               const double* dgd, double* dx, double* du, double* dpred_x, double* dpred_u,
                               int32_t* dskipped, int32_t* dsteps_taken, double* dtraj, int32_t traj_cap,
                               int32_t* dtraj_len, void* stream) {
    return kin_ltv_shift_device(L, veh, B, dsol, dstatus, dAd, dBd, dgd, dx, du, dpred_x, dpred_u, dskipped,
                                dsteps_taken, dtraj, traj_cap, dtraj_len, stream);
}

int mpcqp_kin_shift_vjp_device(const mpcqp_incr_layout* L, const mpcqp_kin_vehicle* veh, int64_t B, const double* dsol,
                               const double* dAd, const double* dBd, const double* dgd, const double* dxt_before,
                               const int32_t* dmode, const double* dgxt, const double* dgpred, const double* dgpdu,
                               double* dgsol, double* dgAd0, double* dgBd0, double* dggd0, double* dgxt_before,
                               void* stream) {
    (void)dgd;  // the step is affine in gd: its VJP does not read it
    return tail_vjp_device<KinIncrTail>("kin_shift_vjp", L, veh, B, dsol, dAd, dBd, dxt_before, dmode, dgxt, nullptr,
                                        dgpred, dgpdu, dgsol, dgAd0, dgBd0, dggd0, dgxt_before, stream);
}

int mpcqp_kin_ltv_shift_vjp_device(const mpcqp_ltv_layout* L, const mpcqp_kin_vehicle* veh, int64_t B,
                                   const double* dsol, const double* dAd, const double* dBd, const double* dx_before,
                                   const int32_t* dmode, const double* dgx, const double* dgu, const double* dgpred_x,
                                   const double* dgpred_u, double* dgsol, double* dgAd0, double* dgBd0, double* dggd0,
                                   double* dgx_before, void* stream) {
    return tail_vjp_device<KinLtvTail>("kin_ltv_shift_vjp", L, veh, B, dsol, dAd, dBd, dx_before, dmode, dgx, dgu,
                                       dgpred_x, dgpred_u, dgsol, dgAd0, dgBd0, dggd0, dgx_before, stream);
}

int mpcqp_kin_reference_search_paths_device(int64_t B, int32_t N, int32_t nxa, int32_t npaths, int32_t npath,
                                            const double* dpaths_x, const double* dpaths_y, const double* dpaths_yaw,
                                            const int32_t* dpath_id, const double* dset_speed, const double* dpred,
                                            double dt, double* dXr, int32_t device, void* stream) {
    if (!dpaths_x || !dpaths_y || !dset_speed || !dpred || !dXr || B < 0 || N < 1 || nxa < 4 || npaths < 1 ||
        npath < 2)
        return set_error(MPCQP_EINVAL, "kin_reference_search_paths: bad arguments");
    if (B == 0) return 0;
    return launch(device, stream, B, 128, k_kin_reference_paths, B, N, nxa, npaths, npath, dpaths_x, dpaths_y,
                  dpaths_yaw, dpath_id, dset_speed, dpred, dt, dXr);
}

int mpcqp_lane_tail_device(const mpcqp_incr_layout* L, const mpcqp_kin_vehicle* veh, int64_t B, const double* dsol,
                           const double* dAd, const double* dBd, const double* dgd, double* dxt, double* dpred,
                           double* dpdu, int32_t nsw, const int32_t* switch_steps, const int32_t* paths_of,
                           int32_t* dstep, int32_t* dpath_id, double* dtraj, int32_t traj_cap, int32_t* dtraj_len,
                           void* stream) {
    return lane_tail_device(L, veh, B, dsol, dAd, dBd, dgd, dxt, dpred, dpdu, nsw, switch_steps, paths_of, dstep,
                            dpath_id, dtraj, traj_cap, dtraj_len, stream);
}

int mpcqp_kin_frozen_tail_device(const mpcqp_ltv_layout* L, int64_t B, const double* dsol, const int32_t* dstatus,
                                 const double* dAd, const double* dBd, const double* dgd, double* dx, double* du,
                                 double* dpred_x, int32_t* dskipped, int32_t* dsteps_taken, double* dtraj,
                                 int32_t traj_cap, int32_t* dtraj_len, void* stream) {
    if (!L || !dsol || !dAd || !dBd || !dgd || !dx || !du || !dpred_x || !dskipped || B < 0 || traj_cap < 0 ||
        (traj_cap > 0 && (!dtraj || !dtraj_len)))
        return set_error(MPCQP_EINVAL, "kin_frozen_tail: bad arguments");
    if (L->nx != 4 || L->nu != 2)
        return set_error(MPCQP_EUNSUPPORTED,
                         "kin_frozen_tail: the plant model is the 4-state kinematic bicycle (nx 4, nu 2)");
    if (B == 0) return 0;
    return launch(L->dev, stream, B, 128, k_kin_frozen_tail, L->N, L->n, B, dsol, dstatus, dAd, dBd, dgd, dx, du,
                  dpred_x, dskipped, dsteps_taken, dtraj, traj_cap, dtraj_len);
}

int mpcqp_lti_step_device(int64_t B, int32_t nxa, int32_t nu, const double* At, const double* Bt, int32_t n,
                          int32_t du_off, int32_t slack_off, const double* dsol, const int32_t* dstatus, double* dxt,
                          int64_t xt_stride, int32_t nsw, const int32_t* switch_steps, const int32_t* regimes,
                          int32_t* dstep, int32_t* dregime, int32_t* dfailed, int32_t* dfail_step, double* dtraj,
                          int32_t traj_cap, int32_t* dtraj_len, int32_t device, void* stream) {
    if (nxa < 1 || nxa > 8 || nu < 1 || nu > 2 || nu > nxa || nsw > 8)
        return set_error(MPCQP_EUNSUPPORTED, "lti_step: need 1 <= nxa <= 8, 1 <= nu <= min(2, nxa), nsw <= 8");
    if (!At || !Bt || !dsol || !dstatus || !dxt || !regimes || !dstep || !dregime || !dfailed || !dfail_step ||
        B < 0 || nsw < 0 || (nsw > 0 && !switch_steps) || n < 1 || du_off < 0 || du_off + nu > n || slack_off >= n ||
        xt_stride < nxa || traj_cap < 0 || (traj_cap > 0 && (!dtraj || !dtraj_len)))
        return set_error(MPCQP_EINVAL, "lti_step: bad arguments");
    if (B == 0) return 0;
    LtiK K = {};
    K.nxa = nxa; K.nu = nu; K.n = n; K.du_off = du_off; K.slack_off = slack_off; K.nsw = nsw;
    std::copy(At, At + nxa * nxa, K.At);
    std::copy(Bt, Bt + nxa * nu, K.Bt);
    std::copy(switch_steps, switch_steps + nsw, K.sw);
    std::copy(regimes, regimes + nsw + 1, K.reg);
    return launch(device, stream, B, 128, k_lti_step, K, B, dsol, dstatus, dxt, xt_stride, dstep, dregime, dfailed,
                  dfail_step, dtraj, traj_cap, dtraj_len);
}

int mpcqp_incr_warm_shift_device(int64_t B, int32_t N, int32_t nxa, int32_t nu, const double* dx, const double* dy,
                                 double* dxs, double* dys, int32_t device, void* stream) {
    if (!dx || !dxs || B < 0 || N < 1 || nxa < 1 || nu < 1 || (!dy) != (!dys) || dx == dxs || (dy && dy == dys))
        return set_error(MPCQP_EINVAL, "incr_warm_shift: bad arguments");
    if (B == 0) return 0;
    const int n = (N + 1) * nxa + N * nu, m = 2 * (N + 1) * nxa + N * nu;
    if (int e = launch(device, stream, B * n, 256, k_stage_shift, B * n, n, N, nxa, nu, 1, dx, dxs)) return e;
    if (dy) return launch(device, stream, B * m, 256, k_stage_shift, B * m, m, N, nxa, nu, 2, dy, dys);
    return 0;
}

// ---- the _fleet twin of every entry point above that takes a vehicle (the same host code over
// the constants' source) ----

int mpcqp_incr_shift_fleet_device(const mpcqp_incr_layout* L, const mpcqp_fleet* f, int64_t B, const double* dsol,
                                  const double* dAd, const double* dBd, const double* dgd, double* dxt, double* dpred,
                                  double* dpdu, void* stream) {
    return incr_shift_device(L, f, B, dsol, dAd, dBd, dgd, dxt, dpred, dpdu, stream);
}

int mpcqp_incr_shift_vjp_fleet_device(const mpcqp_incr_layout* L, const mpcqp_fleet* f, int64_t B, const double* dsol,
                                      const double* dAd, const double* dBd, const double* dgd,
                                      const double* dxt_before, const double* dgxt, const double* dgpred,
                                      const double* dgpdu, double* dgsol, double* dgAd0, double* dgBd0, double* dggd0,
                                      double* dgxt_before, void* stream) {
    (void)dgd;
    return tail_vjp_device<DynamicIncrTail>("incr_shift_vjp_fleet", L, f, B, dsol, dAd, dBd, dxt_before, nullptr, dgxt,
                                            nullptr, dgpred, dgpdu, dgsol, dgAd0, dgBd0, dggd0, dgxt_before, stream);
}

int mpcqp_kin_shift_fleet_device(const mpcqp_incr_layout* L, const mpcqp_kin_fleet* f, int64_t B, const double* dsol,
                                 const double* dAd, const double* dBd, const double* dgd, const double* dXr,
                                 double* dxt, double* dpred, double* dpdu, int32_t* dfinish_cnt, int32_t* ddone,
                                 double* dtraj, int32_t traj_cap, int32_t* dtraj_len, void* stream) {
    return kin_shift_device(L, f, B, dsol, dAd, dBd, dgd, dXr, dxt, dpred, dpdu, dfinish_cnt, ddone, dtraj, traj_cap,
                            dtraj_len, stream);
}

int mpcqp_kin_shift_vjp_fleet_device(const mpcqp_incr_layout* L, const mpcqp_kin_fleet* f, int64_t B,
                                     const double* dsol, const double* dAd, const double* dBd, const double* dgd,
                                     const double* dxt_before, const int32_t* dmode, const double* dgxt,
                                     const double* dgpred, const double* dgpdu, double* dgsol, double* dgAd0,
                                     double* dgBd0, double* dggd0, double* dgxt_before, void* stream) {
    (void)dgd;
    return tail_vjp_device<KinIncrTail>("kin_shift_vjp_fleet", L, f, B, dsol, dAd, dBd, dxt_before, dmode, dgxt,
                                        nullptr, dgpred, dgpdu, dgsol, dgAd0, dgBd0, dggd0, dgxt_before, stream);
}

int mpcqp_kin_rollout_fleet_device(const mpcqp_kin_fleet* f, int64_t B, int32_t N, const double* dx0,
                                   const double* du0, double* dpred_x, double* dpred_u, int32_t device, void* stream) {
    return kin_rollout_device(f, B, N, dx0, du0, dpred_x, dpred_u, device, stream);
}

int mpcqp_kin_ltv_shift_fleet_device(const mpcqp_ltv_layout* L, const mpcqp_kin_fleet* f, int64_t B,
                                     const double* dsol, const int32_t* dstatus, const double* dAd, const double* dBd,
                                     const double* dgd, double* dx, double* du, double* dpred_x, double* dpred_u,
                                     int32_t* dskipped, int32_t* dsteps_taken, double* dtraj, int32_t traj_cap,
                                     int32_t* dtraj_len, void* stream) {
    return kin_ltv_shift_device(L, f, B, dsol, dstatus, dAd, dBd, dgd, dx, du, dpred_x, dpred_u, dskipped,
                                dsteps_taken, dtraj, traj_cap, dtraj_len, stream);
}

int mpcqp_kin_ltv_shift_vjp_fleet_device(const mpcqp_ltv_layout* L, const mpcqp_kin_fleet* f, int64_t B,
                                         const double* dsol, const double* dAd, const double* dBd,
                                         const double* dx_before, const int32_t* dmode, const double* dgx,
                                         const double* dgu, const double* dgpred_x, const double* dgpred_u,
                                         double* dgsol, double* dgAd0, double* dgBd0, double* dggd0,
                                         double* dgx_before, void* stream) {
    return tail_vjp_device<KinLtvTail>("kin_ltv_shift_vjp_fleet", L, f, B, dsol, dAd, dBd, dx_before, dmode, dgx, dgu,
                                       dgpred_x, dgpred_u, dgsol, dgAd0, dgBd0, dggd0, dgx_before, stream);
}

int mpcqp_lane_tail_fleet_device(const mpcqp_incr_layout* L, const mpcqp_kin_fleet* f, int64_t B, const double* dsol,
                                 const double* dAd, const double* dBd, const double* dgd, double* dxt, double* dpred,
                                 double* dpdu, int32_t nsw, const int32_t* switch_steps, const int32_t* paths_of,
                                 int32_t* dstep, int32_t* dpath_id, double* dtraj, int32_t traj_cap,
                                 int32_t* dtraj_len, void* stream) {
    return lane_tail_device(L, f, B, dsol, dAd, dBd, dgd, dxt, dpred, dpdu, nsw, switch_steps, paths_of, dstep,
                            dpath_id, dtraj, traj_cap, dtraj_len, stream);
}

}  // extern "C"
