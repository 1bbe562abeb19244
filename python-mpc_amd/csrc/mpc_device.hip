// mpc_device.hip -- the MPC data path around the solver, on the device
// (SURVEY.md §8f rows F1-F3): everything the reference does in Python between two
// osqp solves of Control/MPC/mpc_dynamics.py:main, batched over B vehicles.
//
//   F2  k_linearise<DynamicBicycle>   Vehicle_Dynamics.get_dynamics_model  vehicle_models.py:52-340
//   F1  k_incr_assemble_A / _vec      mpc_increment's QP values            mpc_dynamics.py:281-389
//   F3  k_reference<DynamicBicycle>   reference_search / nearest_point      mpc_dynamics.py:30-90
//       k_incr_shift                  plant step + horizon shift             mpc_dynamics.py:578-617
//                                     (terminal state: update_dynamics_model vehicle_models.py:343-477)
// and the same loop of Control/MPC/mpc_incre_kine_func.py:simulate on the kinematic bicycle:
//       k_linearise<KinematicBicycle> Vehicle_Kinematics.get_kinematics_model vehicle_models.py:835-863
//       k_reference<KinematicBicycle> reference_search / nearest_point        mpc_incre_kine_func.py:28-81
//       k_kin_shift                   record, stop rule, plant step, shift    mpc_incre_kine_func.py:382-428
// and the LTV MPC in the inputs themselves (mpcqp_ltv_layout: the same layout with nxa = nx, the
// same two assembly kernels), with the closed loop of Control/MPC/mpc_kinematics_pred_matrix.py:main:
//       k_kin_rollout                 initial horizon (nonlinear Euler)       :405-419
//       k_kin_ltv_shift               skip rule, record, plant step, shift    :479-563
// and the two remaining loops of Control/MPC: mpc_increment_kinematics_pred_matrix.py:main (the
// double lane change: a bank of paths, one selected per vehicle by a step schedule) and
// mpc_kinematics.py:main (one linearisation per step for every stage, no shift):
//       k_kin_reference_paths         reference_search on path_id[b] of a path bank   :41-83
//       k_lane_tail                   record, plant step, shift, path schedule        :380-391, :423-472
//       k_kin_frozen_tail             skip rule, unpack, record, plant step           mpc_kinematics.py:397-456
// and the one closed loop that keeps its problem alive, vehicle_lateral_mpc_slack_increment.py
// (setup once, update(q, l, u) + warm-started solve per step; k_affine assembles its vectors):
//       k_lti_step                    raise rule, record, plant step, schedule :158-172, :252-269
// and the gradients with respect to the vehicle's constants, in fleet form:
//       k_linearise_pvjp / k_kin_linearise_pvjp   the linearisations, summed over the stages
//       k_euler_step_pvjp / k_kin_update_pvjp     the terminal steps of the three loop tails
// The two bicycles are model structs (DynamicBicycle, KinematicBicycle) over which the
// linearisation and the reference walk are written once; the three shift kernels share the plant
// step, the trajectory append and kin_update, and keep their own shift and terminal-state rules.
//
// One thread per (vehicle, stage) for the linearisation and per vehicle for the
// sequential parts (reference search walks the path, the shift reorders the
// horizon); one thread per (vehicle, A entry) for the assembly, which is a
// scatter of stage blocks into the shared CSC pattern.  All fp64.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../include/mpcqp.h"
#include "kernels.h"

namespace mpcqp {

// ------------------------------------------------------------------- vehicle --
// Constants of Vehicle_Dynamics (vehicle_models.py:27-50) and of its lateral
// Pacejka tyre model (vehicle_models.py:114-132: B in 1/rad, C, D per axle),
// derived once on the host with the reference's own formulas.
struct VehicleK {
    double m, lf, lr, Iz, dt, cda;  // cda = roh * C_d * A_f
    double roll;                    // C_roll * m * 9.81
    double Bf, Cf, Df, Br, Cr, Dr;
};

// Written once over the scalar S of the nine constructor arguments p = (m, l_f, l_r, width, length,
// C_d, A_f, C_roll, dt), the struct's field order: double for the forward, a 9-wide dual for
// mpcqp_vehicle_constants_vjp.  k: the thirteen constants in VehicleK's order.
template <class S>
static void derive_constants(const S* p, S* k) {
    using std::atan;
    using std::sin;
    const S &m = p[0], &l_f = p[1], &l_r = p[2], &width = p[3], &length = p[4], &C_d = p[5], &A_f = p[6],
            &C_roll = p[7], &dt = p[8];
    k[0] = m; k[1] = l_f; k[2] = l_r; k[4] = dt;
    k[3] = 1.0 / 12 * m * (width * width + length * length);
    const double roh = 1.23;
    k[5] = roh * C_d * A_f;
    k[6] = C_roll * m * 9.81;
    const double a[8] = {-22.1, 1011, 1078, 1.82, 0.208, 0.000, -0.354, 0.707};
    const S wheelbase = l_f + l_r;
    const double pi = 3.141592653589793;
    for (int axle = 0; axle < 2; ++axle) {
        const S Fz = 9.81 * (m * (axle == 0 ? l_r : l_f) / wheelbase) * 0.001;
        const S C = S(1.30);
        const S D = a[0] * Fz * Fz + a[1] * Fz;
        const S BCD = a[2] * sin(a[3] * atan(a[4] * Fz));
        const S B = BCD / (C * D) * 180 / pi;
        k[7 + 3 * axle] = B; k[8 + 3 * axle] = C; k[9 + 3 * axle] = D;
    }
}

static VehicleK vehicle_constants(const mpcqp_vehicle& v) {
    static_assert(sizeof(VehicleK) == 13 * sizeof(double) && sizeof(mpcqp_vehicle) == 9 * sizeof(double),
                  "thirteen constants of nine arguments");
    double p[9], kk[13];
    std::memcpy(p, &v, sizeof(p));
    derive_constants(p, kk);
    VehicleK k;
    std::memcpy(&k, kk, sizeof(k));
    return k;
}
static const mpcqp_kin_vehicle& vehicle_constants(const mpcqp_kin_vehicle& v) { return v; }  // nothing derived

// Where a kernel's constants come from: the struct itself, by value, one car for
// the whole batch (uniform; it stays in SGPRs), or a fleet's table, one K per vehicle in batch
// order (array of structs), which thread (b, .) reads through the reference at the point of use.
template <class K>
struct TableK {
    const K* k;
};
template <class K>
__device__ __forceinline__ const K& constants(const K& k, long) { return k; }
template <class K>
__device__ __forceinline__ const K& constants(const TableK<K>& t, long b) { return t.k[b]; }
// A model or a Tail (below) over a fleet: the kernels that are templates over one take M::K by
// value, so the table goes where the struct went; everything else of M is M's.
template <class M>
struct OverFleet : M {
    using K = TableK<typename M::K>;
};

__device__ __forceinline__ double sgn(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

// low-speed guard of get_dynamics_model / update_dynamics_model (vehicle_models.py:143-159),
// on copies: 0 <= vx < 0.5 or -0.5 < vx < 0 -> vy = r = steer = 0 and |vx| >= 0.3
__device__ __forceinline__ void low_speed_guard(double* x, double* u) {
    const double vx = x[3];
    if (vx >= 0.0 && vx < 0.5) {
        x[4] = 0.0; x[5] = 0.0; u[0] = 0.0;
        if (vx < 0.3) x[3] = 0.3;
    }
    if (x[3] > -0.5 && x[3] < 0.0) {
        x[4] = 0.0; x[5] = 0.0; u[0] = 0.0;
        if (x[3] > -0.3) x[3] = -0.3;
    }
}

// Forward-mode dual number with W tangent slots.  Dual, the 6-wide instance, carries the six inputs
// that have derivative through linearise_one: d[] = d/d(yaw, vx, vy, r, steer, accel).  The model
// below is written once over its scalar types: double for the forward kernels, Dual in the point for
// k_linearise_vjp, DualN<W> in the constants (VehicleKD<W>) for the parameter kernels.
template <int W>
struct DualN {
    static constexpr int ND = W;
    double v;
    double d[ND];
    __host__ __device__ explicit DualN(double v_ = 0.0) : v(v_) {
        for (int j = 0; j < ND; ++j) d[j] = 0.0;
    }
    // the input `slot` at value v_; seed 0 where the low-speed guard replaced it by a constant
    __host__ __device__ DualN(double v_, int slot, bool live) : DualN(v_) { d[slot] = live ? 1.0 : 0.0; }
};
using Dual = DualN<6>;
#define DUAL_FN template <int W> __host__ __device__ __forceinline__
DUAL_FN DualN<W> operator-(const DualN<W>& a) {
    DualN<W> o(-a.v);
    for (int j = 0; j < W; ++j) o.d[j] = -a.d[j];
    return o;
}
DUAL_FN DualN<W> operator+(const DualN<W>& a, const DualN<W>& b) {
    DualN<W> o(a.v + b.v);
    for (int j = 0; j < W; ++j) o.d[j] = a.d[j] + b.d[j];
    return o;
}
DUAL_FN DualN<W> operator-(const DualN<W>& a, const DualN<W>& b) {
    DualN<W> o(a.v - b.v);
    for (int j = 0; j < W; ++j) o.d[j] = a.d[j] - b.d[j];
    return o;
}
DUAL_FN DualN<W> operator*(const DualN<W>& a, const DualN<W>& b) {
    DualN<W> o(a.v * b.v);
    for (int j = 0; j < W; ++j) o.d[j] = a.d[j] * b.v + a.v * b.d[j];
    return o;
}
DUAL_FN DualN<W> operator/(const DualN<W>& a, const DualN<W>& b) {
    DualN<W> o(a.v / b.v);
    for (int j = 0; j < W; ++j) o.d[j] = (a.d[j] - o.v * b.d[j]) / b.v;
    return o;
}
DUAL_FN DualN<W> operator+(const DualN<W>& a, double b) {
    DualN<W> o = a;
    o.v = a.v + b;
    return o;
}
DUAL_FN DualN<W> operator+(double a, const DualN<W>& b) {
    DualN<W> o = b;
    o.v = a + b.v;
    return o;
}
DUAL_FN DualN<W> operator-(const DualN<W>& a, double b) {
    DualN<W> o = a;
    o.v = a.v - b;
    return o;
}
DUAL_FN DualN<W> operator*(const DualN<W>& a, double b) {
    DualN<W> o(a.v * b);
    for (int j = 0; j < W; ++j) o.d[j] = a.d[j] * b;
    return o;
}
DUAL_FN DualN<W> operator*(double a, const DualN<W>& b) {
    DualN<W> o(a * b.v);
    for (int j = 0; j < W; ++j) o.d[j] = a * b.d[j];
    return o;
}
// a plain value over or under a dual: only the parameter kernels and the host chain meet these
DUAL_FN DualN<W> operator/(const DualN<W>& a, double b) {
    DualN<W> o(a.v / b);
    for (int j = 0; j < W; ++j) o.d[j] = a.d[j] / b;
    return o;
}
DUAL_FN DualN<W> operator/(double a, const DualN<W>& b) {
    DualN<W> o(a / b.v);
    for (int j = 0; j < W; ++j) o.d[j] = (-o.v * b.d[j]) / b.v;
    return o;
}
// the double overloads stay visible beside the duals' in this namespace
using ::atan;
using ::atan2;
using ::cos;
using ::sin;
// chain rule with the outer derivative dv
DUAL_FN DualN<W> chain(double v, double dv, const DualN<W>& a) {
    DualN<W> o(v);
    for (int j = 0; j < W; ++j) o.d[j] = dv * a.d[j];
    return o;
}
DUAL_FN DualN<W> sin(const DualN<W>& a) { return chain(::sin(a.v), ::cos(a.v), a); }
DUAL_FN DualN<W> cos(const DualN<W>& a) { return chain(::cos(a.v), -::sin(a.v), a); }
DUAL_FN DualN<W> atan(const DualN<W>& a) { return chain(::atan(a.v), 1.0 / (1.0 + a.v * a.v), a); }
DUAL_FN DualN<W> atan2(const DualN<W>& y, const DualN<W>& x) {
    DualN<W> o(::atan2(y.v, x.v));
    const double n = x.v * x.v + y.v * y.v;
    for (int j = 0; j < W; ++j) o.d[j] = (x.v * y.d[j] - y.v * x.d[j]) / n;
    return o;
}
DUAL_FN DualN<W> atan2(const DualN<W>& y, double x) {
    DualN<W> o(::atan2(y.v, x));
    const double n = x * x + y.v * y.v;
    for (int j = 0; j < W; ++j) o.d[j] = (x * y.d[j]) / n;
    return o;
}
template <int W>
__device__ __forceinline__ double sgn(const DualN<W>& a) { return sgn(a.v); }  // derivative 0, as the reference's Jacobian has it
#undef DUAL_FN

// VehicleK over duals in the constants themselves: what the model functions take where the
// derivative is wanted with respect to the vehicle (slot q of a field = d field / d constant q).
template <int W>
struct VehicleKD {
    DualN<W> m, lf, lr, Iz, dt, cda, roll, Bf, Cf, Df, Br, Cr, Dr;
};
// the scalar a model function computes in: the constants' type times the point's
template <class KV, class T>
struct ModelScalarOf {
    using type = T;  // plain constants: the point's scalar
};
template <int W>
struct ModelScalarOf<VehicleKD<W>, double> {
    using type = DualN<W>;
};
template <class KV, class T>
using ModelScalar = typename ModelScalarOf<KV, T>::type;

// f(x, u) of the dynamic bicycle model (vehicle_models.py:238-245 / 470-475), plus the
// tyre quantities the Jacobian needs
template <class T>
struct Tyre {
    T af, ar, Fyf, Fyr, Fx;
};
template <class T, class KV, class R = ModelScalar<KV, T>>
__device__ __forceinline__ Tyre<R> tyre_forces(const KV& k, const T* x, const T* u) {
    Tyre<R> t;
    const T vx = x[3], vy = x[4], r = x[5], st = u[0], acc = u[1];
    t.af = -atan2(k.lf * r + vy, vx) + st;
    t.ar = -atan2(-k.lr * r + vy, vx);
    t.Fyf = k.Df * sin(k.Cf * atan(k.Bf * t.af));
    t.Fyr = k.Dr * sin(k.Cr * atan(k.Br * t.ar));
    const auto R_roll = k.roll * sgn(vx);
    const R F_aero = 0.5 * k.cda * vx * vx * sgn(vx);
    t.Fx = k.m * acc - F_aero - R_roll;
    return t;
}
template <class T, class KV, class R>
__device__ __forceinline__ void dynamics(const KV& k, const T* x, const T* u, const Tyre<R>& t, R* f) {
    const T yaw = x[2], vx = x[3], vy = x[4], r = x[5], st = u[0];
    const T cy = cos(yaw), sy = sin(yaw), cs = cos(st), ss = sin(st);
    f[0] = R(vx * cy - vy * sy);
    f[1] = R(vy * cy + vx * sy);
    f[2] = R(r);
    f[3] = 1. / k.m * (t.Fx * cs - t.Fyf * ss + k.m * vy * r);
    f[4] = 1. / k.m * (t.Fx * ss + t.Fyr + t.Fyf * cs - k.m * vx * r);
    f[5] = 1. / k.Iz * (t.Fx * k.lf * ss + t.Fyf * k.lf * cs - t.Fyr * k.lr);
}

// get_dynamics_model's continuous-time pieces at a GUARDED (x, u): f, and the structural entries of
// the reference's Jacobians Ac (6x6) and Bc (6x2; every other entry is the constant 0).  That Ac
// is not everywhere the derivative of that f (dFx/dvx = -cda vx holds for vx > 0 only).  Each
// value goes to `out` as soon as it exists: out.F(i, f_i), out.A(i, j, Ac_ij), out.B(i, j, Bc_ij).
template <class T, class KV, class Out>
__device__ __forceinline__ void continuous_model(const KV& k, const T* x, const T* u, Out& out) {
    using R = ModelScalar<KV, T>;
    const Tyre<R> t = tyre_forces(k, x, u);
    R f[6];
    dynamics(k, x, u, t, f);
    for (int i = 0; i < 6; ++i) out.F(i, f[i]);
    const T yaw = x[2], vx = x[3], vy = x[4], r = x[5], st = u[0];
    const auto m = k.m, Iz = k.Iz, lf = k.lf, lr = k.lr;
    const T cy = cos(yaw), sy = sin(yaw), cs = cos(st), ss = sin(st);
    // :251-270 tyre-force derivatives
    const R dFxf_dvx = -k.cda * vx;
    const auto dFxf_daccel = m;
    const R kf = (k.Bf * k.Cf * k.Df * cos(k.Cf * atan(k.Bf * t.af))) / (1 + k.Bf * k.Bf * t.af * t.af);
    const R kr = (k.Br * k.Cr * k.Dr * cos(k.Cr * atan(k.Br * t.ar))) / (1 + k.Br * k.Br * t.ar * t.ar);
    const R af_num = lf * r + vy, ar_num = -lr * r + vy;
    const R nf = af_num * af_num + vx * vx, nr = ar_num * ar_num + vx * vx;
    const R dFyf_dvx = kf * af_num / nf;
    const R dFyf_dvy = kf * (-vx / nf);
    const R dFyf_dr = kf * (-lf * vx) / nf;
    const R dFyf_dst = kf;
    const R dFyr_dvx = kr * ar_num / nr;
    const R dFyr_dvy = kr * (-vx) / nr;
    const R dFyr_dr = kr * (lr * vx) / nr;
    // :273-292 Jacobians
    out.A(0, 2, -vx * sy - vy * cy); out.A(0, 3, cy); out.A(0, 4, -sy);
    out.A(1, 2, -vy * sy + vx * cy); out.A(1, 3, sy); out.A(1, 4, cy);
    out.A(2, 5, T(1.));
    out.A(3, 3, 1 / m * (dFxf_dvx * cs - dFyf_dvx * ss));
    out.A(3, 4, 1 / m * (-dFyf_dvy * ss + m * r));
    out.A(3, 5, 1 / m * (-dFyf_dr * ss + m * vy));
    out.A(4, 3, 1 / m * (dFxf_dvx * ss + dFyr_dvx + dFyf_dvx * cs - m * r));
    out.A(4, 4, 1 / m * (dFyr_dvy + dFyf_dvy * cs));
    out.A(4, 5, 1 / m * (dFyr_dr + dFyf_dr * cs - m * vx));
    out.A(5, 3, 1 / Iz * (dFxf_dvx * lf * ss + dFyf_dvx * lf * cs - dFyr_dvx * lr));
    out.A(5, 4, 1 / Iz * (dFyf_dvy * lf * cs - dFyr_dvy * lr));
    out.A(5, 5, 1 / Iz * (dFyf_dr * lf * cs - dFyr_dr * lr));
    out.B(3, 0, 1 / m * (-t.Fx * ss - dFyf_dst * ss - t.Fyf * cs));
    out.B(3, 1, 1 / m * (dFxf_daccel * cs));
    out.B(4, 0, 1 / m * (t.Fx * cs + dFyf_dst * cs - t.Fyf * ss));
    out.B(4, 1, 1 / m * (dFxf_daccel * ss));
    out.B(5, 0, 1 / Iz * (t.Fx * lf * cs + dFyf_dst * lf * cs - t.Fyf * lf * ss));
    out.B(5, 1, 1 / Iz * (dFxf_daccel * lf * ss));
}

// get_dynamics_model for one (x, u): Ad = I + dt Ac, Bd = dt Bc, gd = dt (f - Ac x - Bc u)
__device__ void linearise_one(const VehicleK& k, const double* xin, const double* uin, double* __restrict__ Ad,
                              double* __restrict__ Bd, double* __restrict__ gd) {
    double x[6], u[2];
    for (int i = 0; i < 6; ++i) x[i] = xin[i];
    u[0] = uin[0]; u[1] = uin[1];
    low_speed_guard(x, u);
    double f[6], Ac[36] = {0.0}, Bc[12] = {0.0};
    struct {
        double *f, *Ac, *Bc;
        __device__ void F(int i, double v) { f[i] = v; }
        __device__ void A(int i, int j, double v) { Ac[i * 6 + j] = v; }
        __device__ void B(int i, int j, double v) { Bc[i * 2 + j] = v; }
    } store = {f, Ac, Bc};
    continuous_model(k, x, u, store);
    // :294, :318-324
    for (int i = 0; i < 6; ++i) {
        double ax = 0.0;
        for (int j = 0; j < 6; ++j) ax += Ac[i * 6 + j] * x[j];
        const double bu = Bc[i * 2 + 0] * u[0] + Bc[i * 2 + 1] * u[1];
        gd[i] = (f[i] - ax - bu) * k.dt;
        for (int j = 0; j < 6; ++j) Ad[i * 6 + j] = (i == j ? 1.0 : 0.0) + Ac[i * 6 + j] * k.dt;
        Bd[i * 2 + 0] = Bc[i * 2 + 0] * k.dt;
        Bd[i * 2 + 1] = Bc[i * 2 + 1] * k.dt;
    }
}

// update_dynamics_model (vehicle_models.py:343-477): one explicit-Euler step of the
// nonlinear model from the guarded state.  euler_step<T> starts at a GUARDED (x, u), as
// continuous_model does: double for k_incr_shift, Dual for its transpose (euler_step_vjp).
template <class T, class KV, class R>
__device__ __forceinline__ void euler_step(const KV& k, const T* x, const T* u, R* xn) {
    const Tyre<R> t = tyre_forces<T>(k, x, u);
    R f[6];
    dynamics(k, x, u, t, f);
    for (int i = 0; i < 6; ++i) xn[i] = x[i] + f[i] * k.dt;
}
__device__ void euler_step_guarded(const VehicleK& k, const double* xin, const double* uin, double* xn) {
    double x[6], u[2];
    for (int i = 0; i < 6; ++i) x[i] = xin[i];
    u[0] = uin[0]; u[1] = uin[1];
    low_speed_guard(x, u);
    euler_step<double>(k, x, u, xn);
}

// ---------------------------------------------------------- kinematic bicycle --
// Vehicle_Kinematics.get_kinematics_model (vehicle_models.py:835-863) for one (x, u):
// x = (X, Y, v, yaw), u = (steer, accel); the model is already discrete (Ad = A, Bd = B,
// gd = C of the reference).  Every entry of the 4x4 / 4x2 / 4 outputs is written.
__device__ void linearise_one(const mpcqp_kin_vehicle& k, const double* x, const double* u,
                              double* __restrict__ Ad, double* __restrict__ Bd, double* __restrict__ gd) {
    const double v = x[2], yaw = x[3], st = u[0];
    const double dt = k.dt, wb = k.l_f + k.l_r;
    const double cy = cos(yaw), sy = sin(yaw), cs = cos(st);
    for (int i = 0; i < 16; ++i) Ad[i] = 0.0;
    for (int i = 0; i < 8; ++i) Bd[i] = 0.0;
    Ad[0 * 4 + 0] = 1.0; Ad[1 * 4 + 1] = 1.0; Ad[2 * 4 + 2] = 1.0; Ad[3 * 4 + 3] = 1.0;
    Ad[0 * 4 + 2] = dt * cy;
    Ad[0 * 4 + 3] = -dt * v * sy;
    Ad[1 * 4 + 2] = dt * sy;
    Ad[1 * 4 + 3] = dt * v * cy;
    Ad[3 * 4 + 2] = dt * tan(st) / wb;
    Bd[2 * 2 + 1] = dt;
    Bd[3 * 2 + 0] = dt * v / (wb * (cs * cs));
    gd[0] = dt * v * sy * yaw;
    gd[1] = -dt * v * cy * yaw;
    gd[2] = 0.0;
    gd[3] = -dt * v * st / (wb * (cs * cs));
}

// update_kinematics_model (vehicle_models.py:866-883): the reference updates in place, so v
// advances before yaw reads it.  xn may alias x.
__device__ __forceinline__ void kin_update(const mpcqp_kin_vehicle& k, const double* x, const double* u,
                                           double* xn) {
    const double X = x[0], Y = x[1], v = x[2], yaw = x[3];
    const double v1 = v + u[1] * k.dt;
    xn[0] = X + v * cos(yaw) * k.dt;
    xn[1] = Y + v * sin(yaw) * k.dt;
    xn[2] = v1;
    xn[3] = yaw + v1 / (k.l_f + k.l_r) * tan(u[0]) * k.dt;
}

// The transpose of kin_update in closed form: w (4) the cotangent of the new state -> gx (4) of
// (X, Y, v, yaw), gu (2) of (steer, accel).  v enters yaw's row through v1 = v + accel dt.
__device__ __forceinline__ void kin_update_vjp(const mpcqp_kin_vehicle& k, const double* x, const double* u,
                                               const double* w, double* gx, double* gu) {
    const double v = x[2], yaw = x[3], st = u[0];
    const double dt = k.dt, wb = k.l_f + k.l_r;
    const double v1 = v + u[1] * dt;
    const double cy = cos(yaw), sy = sin(yaw), ts = tan(st), cs = cos(st);
    gx[0] = w[0];
    gx[1] = w[1];
    gx[2] = ((w[0] * cy * dt + w[1] * sy * dt) + w[2]) + w[3] * ts * dt / wb;
    gx[3] = (-w[0] * v * sy * dt + w[1] * v * cy * dt) + w[3];
    gu[0] = w[3] * v1 * dt / (wb * (cs * cs));
    gu[1] = w[2] * dt + w[3] * dt * dt * ts / wb;
}

// -------------------------------------------------------------------- models --
// What differs between the two bicycles where a kernel is written once over the model: the
// state width, the constants (which select the linearise_one overload), the state that holds
// the speed, and one column of the reference Xr (rows at `stride` = N+1) for the path index
// `ind`.  path_yaw and set_speed are the kinematic reference's own inputs (null for the
// dynamic one).
struct DynamicBicycle {  // x = (X, Y, yaw, vx, vy, r)
    static constexpr int NX = 6, SPEED = 3;
    using K = VehicleK;
    // (path point, yaw 0, vx 10, vy 0, r 0)   (mpc_dynamics.py:44-90)
    static __device__ void reference_column(double* Xc, int stride, double px, double py, const double*, int,
                                            const double*, long) {
        Xc[0 * stride] = px;
        Xc[1 * stride] = py;
        Xc[2 * stride] = 0.0;
        Xc[3 * stride] = 10.0;
        Xc[4 * stride] = 0.0;
        Xc[5 * stride] = 0.0;
    }
};

struct KinematicBicycle {  // x = (X, Y, v, yaw)
    static constexpr int NX = 4, SPEED = 2;
    using K = mpcqp_kin_vehicle;  // its constants are the C ABI's struct itself
    // (path x, path y, set_speed[b], path_yaw[ind])   (mpc_incre_kine_func.py:42-81)
    static __device__ void reference_column(double* Xc, int stride, double px, double py, const double* path_yaw,
                                            int ind, const double* set_speed, long b) {
        Xc[0 * stride] = px;
        Xc[1 * stride] = py;
        Xc[2 * stride] = set_speed[b];
        Xc[3 * stride] = path_yaw[ind];
    }
};

// one thread per (vehicle, stage); x, u: any strides with a contiguous last axis
template <class M>
__global__ __launch_bounds__(256) void k_linearise(typename M::K k, long B, int N, const double* __restrict__ x,
                                                   long x_sb, long x_sk, const double* __restrict__ u, long u_sb,
                                                   long u_sk, double* __restrict__ Ad, double* __restrict__ Bd,
                                                   double* __restrict__ gd) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * N) return;
    const long b = t / N, s = t - b * N;
    constexpr int nx = M::NX, nu = 2;
    linearise_one(constants(k, b), x + b * x_sb + s * x_sk, u + b * u_sb + s * u_sk, Ad + t * (nx * nx),
                  Bd + t * (nx * nu), gd + t * nx);  // the overload of the model's constants
}

// ------------------------------------------------------- incremental QP layout --
// The QP of mpc_increment (mpc_dynamics.py:281-389) for nxa = nx + nu augmented
// states:  variables (x~_0 .. x~_N, du_0 .. du_{N-1}),
//   A = [ Aeq ; I ],  Aeq = [ -I + subdiag(A~_k) | B~_k shifted one block down ],
//   A~_k = [[Ad_k, Bd_k], [0, I]],  B~_k = [Bd_k; I].
// The pattern keeps every STRUCTURAL nonzero of Ad / Bd (masks), so it does not
// change when a value happens to be 0 (the reference's scipy pattern does; the
// QP is the same -- an explicit zero contributes nothing to OSQP's arithmetic).
// Ax source codes: >= 0 -> Ad entry (stage * nx*nx + i*nx + j); -1 - c -> Bd entry
// c = stage * nx*nu + i*nu + j; kConst -> the template value.
//
// With nxa = nx the same layout is the direct-input LTV QP of mpc__
// (mpc_kinematics_pred_matrix.py:268-352), mpc (mpc_dynamics.py:160-279) and mpc_
// (mpc_kinematics.py:202-265): variables (x_0 .. x_N, u_0 .. u_{N-1}), no augmentation,
//   A = [ Aeq ; I ],  Aeq = [ -I + subdiag(Ad_k) | Bd_k shifted one block down ].
constexpr int kConstSrc = INT32_MIN;

struct IncrLayout {
    int N = 0, nx = 0, nu = 0, nxa = 0, n = 0, m = 0, dev = 0;
    std::vector<int> Pp, Pi, Ap, Ai, asrc;
    // Qt: [2][nx*nx], stage then terminal: the rows i < nx of (Q C)' ([i][j] = Q[j][i]) for the
    // augmented layout, Q itself for nxa = nx (q = -Q Xr_k)
    std::vector<double> Px, Atpl, ltpl, utpl, Qt;
    int* d_asrc = nullptr;
    double *d_Atpl = nullptr, *d_ltpl = nullptr, *d_utpl = nullptr, *d_Qt = nullptr;
    // The reverse maps of the assembly, for its VJP and for weights given per call (indexed at
    // creation, uploaded by the first call that needs them):
    //   adst[N nx nx]: the Ax slot of Ad_k[i][j], -1 where maskA is 0;
    //   bdst[N nx nu][2]: the Ax slots of Bd_k[i][j] in CSC order (one in the LTV layout, two in the
    //     augmented one: A~_k's upper-right block, then B~_k), -1 for none;
    //   W: (Q | QN | R) dense row-major as the caller gave them; psrc[nnzP]: the entry of W a stored
    //     entry of P holds; wptr / wlist: per entry of W the P slots that hold it, ascending.
    std::vector<int> adst, bdst, psrc, wptr, wlist;
    std::vector<double> W;
    int *d_adst = nullptr, *d_bdst = nullptr, *d_psrc = nullptr, *d_wptr = nullptr, *d_wlist = nullptr;
    double *d_W = nullptr, *d_Qtw = nullptr;  // d_Qtw: [2][nx*nx], Qt of the weights of the last *_assemble_w call
};

struct IncrK {  // what the device kernels need (by value)
    int N, nx, nu, nxa, n, m, nnzA;
    const int* asrc;
    const double *Atpl, *ltpl, *utpl, *Qt;  // Qt: [2][nx*nx] (stage weights, terminal weights)
};

__global__ __launch_bounds__(256) void k_incr_assemble_A(IncrK L, long B, const double* __restrict__ Ad,
                                                         const double* __restrict__ Bd, double* __restrict__ Ax) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * L.nnzA) return;
    const long b = t / L.nnzA;
    const int e = (int)(t - b * L.nnzA);
    const int s = L.asrc[e];
    double v;
    if (s == kConstSrc) v = L.Atpl[e];
    else if (s >= 0) v = Ad[b * (long)L.N * L.nx * L.nx + s];
    else v = Bd[b * (long)L.N * L.nx * L.nu + (-1 - s)];
    Ax[t] = v;
}

// q, l, u of one vehicle per thread, for either layout (nxa >= nx):
//   q = [ -W Xr_k (k < N) ; -WN Xr_N ; 0 ],  W = L.Qt rows i < nx, augmented rows -0.0   (:313-319)
//   leq = ueq = [ -x~_0 ; -g~_k ],  g~_k = [gd_k; 0]   (:371-378); inequality rows: the template,
//   but for the state rows where xlo / xhi (may be null; (B, N+1, nxa)) give per-stage bounds
//   (mpc_'s corridor), clipped like the template.
__global__ __launch_bounds__(128) void k_incr_assemble_vec(IncrK L, long B, const double* __restrict__ gd,
                                                           const double* __restrict__ xt0,
                                                           const double* __restrict__ Xr,
                                                           const double* __restrict__ xlo,
                                                           const double* __restrict__ xhi, double* __restrict__ q,
                                                           double* __restrict__ l, double* __restrict__ u) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int N = L.N, nx = L.nx, nxa = L.nxa, n = L.n, m = L.m;
    const double INF = 1e30;
    double* qb = q + b * n;
    const double* Xb = Xr + b * (long)nx * (N + 1);  // Xr[j][k] at j*(N+1)+k
    for (int k = 0; k <= N; ++k) {
        const double* W = L.Qt + (k == N ? nx * nx : 0);
        for (int i = 0; i < nx; ++i) {
            double acc = 0.0;
            for (int j = 0; j < nx; ++j) acc += W[i * nx + j] * Xb[j * (N + 1) + k];
            qb[k * nxa + i] = -acc;
        }
        for (int i = nx; i < nxa; ++i) qb[k * nxa + i] = -0.0;  // the empty sum, negated
    }
    const int ns = (N + 1) * nxa;  // state rows of the box start at ns, input rows at 2 ns
    for (int i = ns; i < n; ++i) qb[i] = 0.0;
    double* lb = l + b * m;
    double* ub = u + b * m;
    for (int i = 0; i < nxa; ++i) lb[i] = ub[i] = -xt0[b * nxa + i];
    const double* gb = gd + b * (long)N * nx;
    for (int k = 0; k < N; ++k) {
        for (int i = 0; i < nx; ++i) lb[(k + 1) * nxa + i] = ub[(k + 1) * nxa + i] = -gb[k * nx + i];
        for (int i = nx; i < nxa; ++i) lb[(k + 1) * nxa + i] = ub[(k + 1) * nxa + i] = -0.0;
    }
    for (int r = ns; r < m; ++r) {
        lb[r] = L.ltpl[r];
        ub[r] = L.utpl[r];
    }
    // per-stage state bounds over the template's (one plain copy loop above: the closed loops,
    // which give none, spend half their data-path time in this kernel)
    if (xlo)
        for (int i = 0; i < ns; ++i) lb[ns + i] = fmin(fmax(xlo[b * (long)ns + i], -INF), INF);
    if (xhi)
        for (int i = 0; i < ns; ++i) ub[ns + i] = fmin(fmax(xhi[b * (long)ns + i], -INF), INF);
}

// ------------------------------------------- the assembly's VJP, weights per call --
// Transposes of the two kernels above (mpcqp_*_assemble_vjp_device): every output element is
// written by one thread, which gathers its contributions in a fixed order -- no atomics, so two
// calls give the same bits.  A null cotangent reads as zero, a null output is not written.
struct VjpK {
    int N, nx, nu, nxa, n, m, nnzA, nnzP, tr;  // tr: W_k[i][j] = Wp[j][i] (the caller's Q under the augmented layout)
    const int *adst, *bdst, *wptr, *wlist;
    const double *Wst, *Wtm;  // stage / terminal weights the forward multiplied with (through tr)
};

// one thread per (instance, entry of Ad_0..Ad_{N-1} then of Bd_0..Bd_{N-1})
__global__ __launch_bounds__(256) void k_assemble_vjp_AB(VjpK L, long B, const double* __restrict__ gAx,
                                                         double* __restrict__ gAd, double* __restrict__ gBd) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int na = L.N * L.nx * L.nx, nb = L.N * L.nx * L.nu, per = na + nb;
    if (t >= B * per) return;
    const long b = t / per;
    const int e = (int)(t - b * per);
    const double* g = gAx ? gAx + b * L.nnzA : nullptr;
    if (e < na) {
        if (!gAd) return;
        const int s = L.adst[e];
        gAd[b * na + e] = (g && s >= 0) ? g[s] : 0.0;
    } else {
        if (!gBd) return;
        const int c = e - na, s0 = L.bdst[2 * c], s1 = L.bdst[2 * c + 1];
        double v = 0.0;
        if (g && s0 >= 0) v = s1 >= 0 ? g[s0] + g[s1] : g[s0];
        gBd[b * nb + c] = v;
    }
}

// one thread per (instance, element of ggd | gx0 | gXr | gxlo | gxhi)
__global__ __launch_bounds__(256) void k_assemble_vjp_vec(VjpK L, long B, const double* __restrict__ gq,
                                                          const double* __restrict__ gl,
                                                          const double* __restrict__ gu,
                                                          const double* __restrict__ xlo,
                                                          const double* __restrict__ xhi, double* __restrict__ ggd,
                                                          double* __restrict__ gx0, double* __restrict__ gXr,
                                                          double* __restrict__ gxlo, double* __restrict__ gxhi) {
    const int N = L.N, nx = L.nx, nxa = L.nxa, ns = (N + 1) * nxa;
    const int n0 = N * nx, n1 = n0 + nxa, n2 = n1 + nx * (N + 1), n3 = n2 + ns, per = n3 + ns;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * per) return;
    const long b = t / per;
    const int e = (int)(t - b * per);
    const double INF = 1e30;
    const double* lb = gl ? gl + b * L.m : nullptr;
    const double* ub = gu ? gu + b * L.m : nullptr;
    if (e < n1) {  // the equality rows: l = u = (-x~_0; -g~_k)
        const int k = e / nx, i = e - k * nx;
        const int row = e < n0 ? (k + 1) * nxa + i : e - n0;
        const double v = -((lb ? lb[row] : 0.0) + (ub ? ub[row] : 0.0));
        if (e < n0) { if (ggd) ggd[b * n0 + e] = v; }
        else if (gx0) gx0[b * nxa + (e - n0)] = v;
    } else if (e < n2) {  // q_k = -W_k Xr_k
        if (!gXr) return;
        const int c = e - n1, j = c / (N + 1), k = c - j * (N + 1);
        const double* W = k == N ? L.Wtm : L.Wst;
        double acc = 0.0;
        if (gq)
            for (int i = 0; i < nx; ++i) acc += W[L.tr ? j * nx + i : i * nx + j] * gq[b * L.n + k * nxa + i];
        gXr[b * (long)nx * (N + 1) + c] = -acc;
    } else if (e < n3) {  // the state rows of the box where the forward did not clip
        if (!gxlo) return;
        const int i = e - n2;
        const double x = xlo[b * (long)ns + i];
        gxlo[b * (long)ns + i] = (lb && x > -INF && x < INF) ? lb[ns + i] : 0.0;
    } else {
        if (!gxhi) return;
        const int i = e - n3;
        const double x = xhi[b * (long)ns + i];
        gxhi[b * (long)ns + i] = (ub && x > -INF && x < INF) ? ub[ns + i] : 0.0;
    }
}

// one thread per (instance, entry of gQ | gQN | gR): the stored entries of P that hold it, summed
// in stage order, minus sum_k gq_k (x) Xr_k through the forward's own W
__global__ __launch_bounds__(256) void k_assemble_vjp_w(VjpK L, long B, const double* __restrict__ gPx,
                                                        const double* __restrict__ gq,
                                                        const double* __restrict__ Xr, double* __restrict__ gQ,
                                                        double* __restrict__ gQN, double* __restrict__ gR) {
    const int N = L.N, nx = L.nx, nu = L.nu, nxa = L.nxa, nq = nx * nx, per = 2 * nq + nu * nu;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * per) return;
    const long b = t / per;
    const int w = (int)(t - b * per);
    double* out = w < nq ? gQ : (w < 2 * nq ? gQN : gR);
    if (!out) return;
    double pp = 0.0;
    if (gPx)
        for (int s = L.wptr[w]; s < L.wptr[w + 1]; ++s) pp += gPx[b * L.nnzP + L.wlist[s]];
    if (w >= 2 * nq) {
        out[b * (nu * nu) + (w - 2 * nq)] = pp;
        return;
    }
    const int el = w < nq ? w : w - nq, r = el / nx, c = el - r * nx;
    const int gi = L.tr ? c : r, xj = L.tr ? r : c;  // d q_k[gi] / d Q[r][c] = -Xr[xj][k]
    double qq = 0.0;
    if (gq && Xr) {
        const double* Xb = Xr + b * (long)nx * (N + 1);
        const double* qb = gq + b * L.n;
        if (w < nq)
            for (int k = 0; k < N; ++k) qq += qb[k * nxa + gi] * Xb[xj * (N + 1) + k];
        else
            qq = qb[N * nxa + gi] * Xb[xj * (N + 1) + N];
    }
    out[b * nq + el] = pp - qq;
}

// Weights given per call (mpcqp_*_assemble_w_device): the Qt-form scratch k_incr_assemble_vec
// reads, and P's stored values in the pattern fixed at creation.  One thread per entry.
__global__ __launch_bounds__(256) void k_weights(int nx, int nnzP, int tr, const int* __restrict__ psrc,
                                                 const double* __restrict__ Q, const double* __restrict__ QN,
                                                 const double* __restrict__ R, double* __restrict__ Qt,
                                                 double* __restrict__ Px) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, nq = nx * nx;
    if (t < 2 * nq) {
        const int el = t < nq ? t : t - nq, i = el / nx, j = el - i * nx;
        Qt[t] = (t < nq ? Q : QN)[tr ? j * nx + i : i * nx + j];
    } else if (t < 2 * nq + nnzP) {
        if (!Px) return;
        const int e = t - 2 * nq, s = psrc[e];
        Px[e] = s < nq ? Q[s] : (s < 2 * nq ? QN[s - nq] : R[s - 2 * nq]);
    }
}

// VJP of linearise_one(const mpcqp_kin_vehicle&, ...) per (vehicle, stage): only v, yaw and steer
// carry derivative; the outputs are dense (B, N, 4) / (B, N, 2) whatever the input strides.
// A template over the constants' source KS (the struct, or a fleet's TableK), as every kernel of
// this file that takes a vehicle and is not a template over its model or Tail already.
template <class KS>
__global__ __launch_bounds__(256) void k_kin_linearise_vjp(KS ks, long B, int N, const double* __restrict__ x,
                                                           long x_sb, long x_sk, const double* __restrict__ u,
                                                           long u_sb, long u_sk, const double* __restrict__ gAd,
                                                           const double* __restrict__ gBd,
                                                           const double* __restrict__ ggd, double* __restrict__ gx,
                                                           double* __restrict__ gu) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * N) return;
    const long b = t / N, s = t - b * N;
    const mpcqp_kin_vehicle& k = constants(ks, b);
    const double* xs = x + b * x_sb + s * x_sk;
    const double v = xs[2], yaw = xs[3], st = u[b * u_sb + s * u_sk];
    const double dt = k.dt, wb = k.l_f + k.l_r;
    const double cy = cos(yaw), sy = sin(yaw), cs = cos(st), ss = sin(st);
    const double sec2 = 1.0 / (cs * cs), dsec2 = 2.0 * ss / (cs * cs * cs);
    const double* A = gAd ? gAd + t * 16 : nullptr;
    const double a02 = A ? A[0 * 4 + 2] : 0.0, a03 = A ? A[0 * 4 + 3] : 0.0, a12 = A ? A[1 * 4 + 2] : 0.0,
                 a13 = A ? A[1 * 4 + 3] : 0.0, a32 = A ? A[3 * 4 + 2] : 0.0;
    const double b30 = gBd ? gBd[t * 8 + 3 * 2 + 0] : 0.0;
    const double g0 = ggd ? ggd[t * 4 + 0] : 0.0, g1 = ggd ? ggd[t * 4 + 1] : 0.0, g3 = ggd ? ggd[t * 4 + 3] : 0.0;
    if (gx) {
        const double gv = dt * ((a13 * cy - a03 * sy) + (g0 * sy - g1 * cy) * yaw + (b30 - g3 * st) * sec2 / wb);
        const double gyaw = dt * ((a12 * cy - a02 * sy) - v * (a03 * cy + a13 * sy) +
                                  v * (g0 * (cy * yaw + sy) + g1 * (sy * yaw - cy)));
        gx[t * 4 + 0] = 0.0;
        gx[t * 4 + 1] = 0.0;
        gx[t * 4 + 2] = gv;
        gx[t * 4 + 3] = gyaw;
    }
    if (gu) {
        gu[t * 2 + 0] = dt / wb * (a32 * sec2 + v * (b30 * dsec2 - g3 * (sec2 + st * dsec2)));
        gu[t * 2 + 1] = 0.0;
    }
}

// What k_linearise_vjp does with each value of continuous_model, a Dual: its tangent goes into the
// sum g[] with the weight of everything the forward made of it,
//   Ad_ij = delta_ij + dt Ac_ij,  Bd_ij = dt Bc_ij,  gd_i = dt (f_i - sum_j Ac_ij x_j - sum_j Bc_ij u_j),
// so nothing but g[], the point and the cotangents of one row stays live.
struct VjpFold {
    const Dual *x, *u;
    const double *gAd, *gBd;  // this thread's 36 / 12, or null
    double ggd[6], dt;
    double g[Dual::ND];
    __device__ void fold(const Dual& o, double c) {
        for (int q = 0; q < Dual::ND; ++q) g[q] += c * o.d[q];
    }
    __device__ void F(int i, const Dual& v) { fold(v, ggd[i] * dt); }
    __device__ void A(int i, int j, const Dual& v) {
        if (gAd) fold(v, gAd[i * 6 + j] * dt);
        fold(v * x[j], -(ggd[i] * dt));
    }
    __device__ void B(int i, int j, const Dual& v) {
        if (gBd) fold(v, gBd[i * 2 + j] * dt);
        fold(v * u[j], -(ggd[i] * dt));
    }
};

// VJP of linearise_one(const VehicleK&, ...) per (vehicle, stage), of the forward as it is
// written: the low-speed guard first (what it replaces by a constant carries no derivative), then
// continuous_model over forward-mode duals in (yaw, vx, vy, r, steer, accel), each output's
// tangent contracted with its cotangent as soon as it exists.  Outputs dense (B, N, 6) / (B, N, 2).
template <class KS>
__global__ __launch_bounds__(256) void k_linearise_vjp(KS ks, long B, int N, const double* __restrict__ x, long x_sb,
                                                       long x_sk, const double* __restrict__ u, long u_sb, long u_sk,
                                                       const double* __restrict__ gAd, const double* __restrict__ gBd,
                                                       const double* __restrict__ ggd, double* __restrict__ gx,
                                                       double* __restrict__ gu) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * N) return;
    const long b = t / N, s = t - b * N;
    // By value: read through the table's pointer, the constants are loaded again at every use over
    // these six thousand instructions, 1 / m and 1 / Iz are formed again with them, and the
    // products contract with other sums than in the uniform form -- other bits.
    const VehicleK k = constants(ks, b);
    const double* xin = x + b * x_sb + s * x_sk;
    const double* uin = u + b * u_sb + s * u_sk;
    double xg[6], ug[2];
    for (int i = 0; i < 6; ++i) xg[i] = xin[i];
    ug[0] = uin[0]; ug[1] = uin[1];
    const double vx_in = xg[3];
    low_speed_guard(xg, ug);
    // the guard's two regions: |vx| < 0.5 replaces vy, r, steer; |vx| < 0.3 replaces vx as well
    const bool lat = !(vx_in > -0.5 && vx_in < 0.5), lon = !(vx_in > -0.3 && vx_in < 0.3);
    const Dual xd[6] = {Dual(xg[0]),          Dual(xg[1]),         Dual(xg[2], 0, true),
                        Dual(xg[3], 1, lon), Dual(xg[4], 2, lat), Dual(xg[5], 3, lat)};
    const Dual ud[2] = {Dual(ug[0], 4, lat), Dual(ug[1], 5, true)};
    VjpFold out = {xd, ud, gAd ? gAd + t * 36 : nullptr, gBd ? gBd + t * 12 : nullptr};
    for (int i = 0; i < 6; ++i) out.ggd[i] = ggd ? ggd[t * 6 + i] : 0.0;
    out.dt = k.dt;
    for (int q = 0; q < Dual::ND; ++q) out.g[q] = 0.0;
    continuous_model(k, xd, ud, out);
    const double* g = out.g;
    if (gx) {
        gx[t * 6 + 0] = 0.0;
        gx[t * 6 + 1] = 0.0;
        gx[t * 6 + 2] = g[0];
        gx[t * 6 + 3] = lon ? g[1] : 0.0;
        gx[t * 6 + 4] = lat ? g[2] : 0.0;
        gx[t * 6 + 5] = lat ? g[3] : 0.0;
    }
    if (gu) {
        gu[t * 2 + 0] = lat ? g[4] : 0.0;
        gu[t * 2 + 1] = g[5];
    }
}

// ------------------------------------------- gradients of the vehicle's constants --
// DESIGN.md §25.  The cotangent of a fleet's table has the table's shape: gK (B, 13) in VehicleK's
// order (m, l_f, l_r, Iz, dt, cda, roll, B_f, C_f, D_f, B_r, C_r, D_r), (B, 3) in
// mpcqp_kin_vehicle's (l_f, l_r, dt).  Fleet form only: a uniform vehicle is a fleet of copies whose
// rows the caller sums.  The rules are k_linearise_vjp's: the guard first, what it replaced is a
// constant (the point carries no tangent here at all), sgn has derivative 0, Ac as written.

// The constants C0 .. C0 + W - 1 of VehicleK's order seeded in slots 0 .. W - 1, the others plain.
template <int C0, int W>
__device__ __forceinline__ VehicleKD<W> seed_constants(const VehicleK& k) {
    const auto sd = [](double v, int c) {
        return (c >= C0 && c < C0 + W) ? DualN<W>(v, c - C0, true) : DualN<W>(v);
    };
    VehicleKD<W> d;
    d.m = sd(k.m, 0); d.lf = sd(k.lf, 1); d.lr = sd(k.lr, 2); d.Iz = sd(k.Iz, 3); d.dt = sd(k.dt, 4);
    d.cda = sd(k.cda, 5); d.roll = sd(k.roll, 6);
    d.Bf = sd(k.Bf, 7); d.Cf = sd(k.Cf, 8); d.Df = sd(k.Df, 9);
    d.Br = sd(k.Br, 10); d.Cr = sd(k.Cr, 11); d.Dr = sd(k.Dr, 12);
    return d;
}
constexpr int kDtSlot = 4;  // dt's place in VehicleK's order

// VjpFold's twin for the constants.  continuous_model hands it values that are duals in the
// constants (or plain doubles, where no constant enters); the point (x, u) is plain.  With c the
// cotangent's weight without dt (gAd_ij, gBd_ij, ggd_i, -ggd_i x_j, -ggd_i u_j):
//   g[q] += (c dt) d value / d constant q      -- VjpFold's weights
//   gdt  += c value                            -- Ad = I + dt Ac, Bd = dt Bc, gd = dt (...) in dt itself
template <int W>
struct PvjpFold {
    const double *x, *u;      // the guarded point
    const double *gAd, *gBd;  // this thread's 36 / 12, or null
    double ggd[6], dt;
    double g[W], gdt;
    __device__ void fold(const DualN<W>& o, double c) {
        const double cw = c * dt;
        for (int q = 0; q < W; ++q) g[q] += cw * o.d[q];
        gdt += c * o.v;
    }
    __device__ void fold(double o, double c) { gdt += c * o; }
    template <class S>
    __device__ void F(int i, const S& v) { fold(v, ggd[i]); }
    template <class S>
    __device__ void A(int i, int j, const S& v) {
        if (gAd) fold(v, gAd[i * 6 + j]);
        fold(v * x[j], -ggd[i]);
    }
    template <class S>
    __device__ void B(int i, int j, const S& v) {
        if (gBd) fold(v, gBd[i * 2 + j]);
        fold(v * u[j], -ggd[i]);
    }
};

// The deterministic stage sum of the two linearisation kernels.  A block of 256 threads holds
// vpb = 256 / N whole vehicles, thread lv * N + s = (vehicle lv of the block, stage s); its W
// partials go to LDS as part[q * 256 + thread], and element (lv, q) is summed by ONE thread in stage
// order, acc = 0, acc += part[s] for s = 0 .. N-1, and written once.  No atomics; N <= 256.
template <int W, class Write>
__device__ __forceinline__ void stage_sum(double* part, const double* g, bool live, int N, int vpb, long B,
                                          Write write) {
    if (live)
        for (int q = 0; q < W; ++q) part[q * 256 + threadIdx.x] = g[q];
    __syncthreads();
    for (int e = threadIdx.x; e < vpb * W; e += 256) {
        const int lv = e / W, q = e - lv * W;
        const long b = (long)blockIdx.x * vpb + lv;
        if (b >= B) break;
        double acc = 0.0;
        for (int s = 0; s < N; ++s) acc += part[q * 256 + lv * N + s];
        write(b, q, acc);
    }
}

// d (Ad, Bd, gd of linearise_one) / d constants C0 .. C0 + W - 1, contracted with (gAd, gBd, ggd)
// and summed over the N stages: gK[b * 13 + C0 + q].  Two instantiations cover the thirteen,
// <0, 7> = (m, l_f, l_r, Iz, dt, cda, roll) and <7, 6> = the tyre constants, so that the tangents fit
// the register file.  Fleet form only; grid = ceil(B / vpb) blocks of 256.
template <int C0, int W>
__global__ __launch_bounds__(256) void k_linearise_pvjp(TableK<VehicleK> ks, long B, int N, int vpb,
                                                        const double* __restrict__ x, long x_sb, long x_sk,
                                                        const double* __restrict__ u, long u_sb, long u_sk,
                                                        const double* __restrict__ gAd,
                                                        const double* __restrict__ gBd,
                                                        const double* __restrict__ ggd, double* __restrict__ gK) {
    __shared__ double part[W * 256];
    const int lv = threadIdx.x / N, s = threadIdx.x - lv * N;
    const long b = (long)blockIdx.x * vpb + lv;
    const bool live = lv < vpb && b < B;
    double g[W];
    for (int q = 0; q < W; ++q) g[q] = 0.0;
    if (live) {
        const long t = b * N + s;
        const VehicleK k = constants(ks, b);  // by value, as k_linearise_vjp
        const double* xin = x + b * x_sb + s * x_sk;
        const double* uin = u + b * u_sb + s * u_sk;
        double xg[6], ug[2];
        for (int i = 0; i < 6; ++i) xg[i] = xin[i];
        ug[0] = uin[0]; ug[1] = uin[1];
        low_speed_guard(xg, ug);
        const VehicleKD<W> kd = seed_constants<C0, W>(k);
        PvjpFold<W> out = {xg, ug, gAd ? gAd + t * 36 : nullptr, gBd ? gBd + t * 12 : nullptr};
        for (int i = 0; i < 6; ++i) out.ggd[i] = ggd ? ggd[t * 6 + i] : 0.0;
        out.dt = k.dt;
        for (int q = 0; q < W; ++q) out.g[q] = 0.0;
        out.gdt = 0.0;
        continuous_model(kd, xg, ug, out);
        for (int q = 0; q < W; ++q) g[q] = out.g[q];
        if constexpr (kDtSlot >= C0 && kDtSlot < C0 + W) g[kDtSlot - C0] = out.gdt;  // no model value reads dt
    }
    stage_sum<W>(part, g, live, N, vpb, B, [&](long bb, int q, double v) { gK[bb * 13 + C0 + q] = v; });
}

// The same for linearise_one(const mpcqp_kin_vehicle&, ...), in closed form as k_kin_linearise_vjp
// is: every structural entry is dt times a function of the point and 1 / wb, wb = l_f + l_r, so
// gK[b] = (g_wb, g_wb, g_dt) summed over the stages.
__global__ __launch_bounds__(256) void k_kin_linearise_pvjp(TableK<mpcqp_kin_vehicle> ks, long B, int N, int vpb,
                                                            const double* __restrict__ x, long x_sb, long x_sk,
                                                            const double* __restrict__ u, long u_sb, long u_sk,
                                                            const double* __restrict__ gAd,
                                                            const double* __restrict__ gBd,
                                                            const double* __restrict__ ggd,
                                                            double* __restrict__ gK) {
    __shared__ double part[2 * 256];
    const int lv = threadIdx.x / N, s = threadIdx.x - lv * N;
    const long b = (long)blockIdx.x * vpb + lv;
    const bool live = lv < vpb && b < B;
    double g[2] = {0.0, 0.0};  // (wb, dt)
    if (live) {
        const long t = b * N + s;
        const mpcqp_kin_vehicle& k = constants(ks, b);
        const double* xs = x + b * x_sb + s * x_sk;
        const double v = xs[2], yaw = xs[3], st = u[b * u_sb + s * u_sk];
        const double dt = k.dt, wb = k.l_f + k.l_r;
        const double cy = cos(yaw), sy = sin(yaw), cs = cos(st), ts = tan(st);
        const double sec2 = 1.0 / (cs * cs);
        const double* A = gAd ? gAd + t * 16 : nullptr;
        const double a02 = A ? A[0 * 4 + 2] : 0.0, a03 = A ? A[0 * 4 + 3] : 0.0, a12 = A ? A[1 * 4 + 2] : 0.0,
                     a13 = A ? A[1 * 4 + 3] : 0.0, a32 = A ? A[3 * 4 + 2] : 0.0;
        const double b21 = gBd ? gBd[t * 8 + 2 * 2 + 1] : 0.0, b30 = gBd ? gBd[t * 8 + 3 * 2 + 0] : 0.0;
        const double g0 = ggd ? ggd[t * 4 + 0] : 0.0, g1 = ggd ? ggd[t * 4 + 1] : 0.0,
                     g3 = ggd ? ggd[t * 4 + 3] : 0.0;
        // what 1 / wb multiplies, without dt
        const double over_wb = a32 * ts + (b30 - g3 * st) * v * sec2;
        g[0] = -(dt * over_wb) / (wb * wb);
        g[1] = ((a02 * cy + a12 * sy) + v * (a13 * cy - a03 * sy)) + b21 + v * yaw * (g0 * sy - g1 * cy) +
               over_wb / wb;
    }
    stage_sum<2>(part, g, live, N, vpb, B, [&](long bb, int q, double v) {
        if (q == 0) gK[bb * 3 + 0] = gK[bb * 3 + 1] = v;
        else gK[bb * 3 + 2] = v;
    });
}

// d euler_step_guarded / d constants C0 .. C0 + W - 1, contracted with w (6): the Euler step over
// duals in the constants from the guarded point; dt is one of them (xn = x + f dt).
template <int C0, int W>
__device__ __forceinline__ void euler_step_pvjp_group(const VehicleK& k, const double* xg, const double* ug,
                                                      const double* w, double* gk) {
    const VehicleKD<W> kd = seed_constants<C0, W>(k);
    DualN<W> xe[6];
    euler_step<double>(kd, xg, ug, xe);
    for (int q = 0; q < W; ++q) {
        double acc = 0.0;
        for (int i = 0; i < 6; ++i) acc += w[i] * xe[i].d[q];
        gk[C0 + q] = acc;
    }
}

// The terminal step of k_incr_shift with respect to the constants, one thread per vehicle: x (6)
// and u (2) at a batch stride (views into the taped solution), w (B, 6) the cotangent of the new
// state (null = zero), mode (null = 0 everywhere): a vehicle whose mode is not 0 did not take the
// step and gets a zero row.  gK (B, 13), every element written.
__global__ __launch_bounds__(128) void k_euler_step_pvjp(TableK<VehicleK> ks, long B, const double* __restrict__ x,
                                                         long x_sb, const double* __restrict__ u, long u_sb,
                                                         const double* __restrict__ w,
                                                         const int* __restrict__ mode, double* __restrict__ gK) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double gk[13];
    for (int c = 0; c < 13; ++c) gk[c] = 0.0;
    if (w && !(mode && mode[b] != 0)) {
        const VehicleK k = constants(ks, b);
        double xg[6], ug[2], wb[6];
        for (int i = 0; i < 6; ++i) xg[i] = x[b * x_sb + i];
        ug[0] = u[b * u_sb + 0]; ug[1] = u[b * u_sb + 1];
        for (int i = 0; i < 6; ++i) wb[i] = w[b * 6 + i];
        low_speed_guard(xg, ug);
        euler_step_pvjp_group<0, 7>(k, xg, ug, wb, gk);
        euler_step_pvjp_group<7, 6>(k, xg, ug, wb, gk);
    }
    for (int c = 0; c < 13; ++c) gK[b * 13 + c] = gk[c];
}

// The same for kin_update (the terminal step of the three kinematic tails), in closed form:
// x (4), u (2) at a batch stride, w (B, 4); gK (B, 3) = (g_wb, g_wb, g_dt).
__global__ __launch_bounds__(128) void k_kin_update_pvjp(TableK<mpcqp_kin_vehicle> ks, long B,
                                                         const double* __restrict__ x, long x_sb,
                                                         const double* __restrict__ u, long u_sb,
                                                         const double* __restrict__ w,
                                                         const int* __restrict__ mode, double* __restrict__ gK) {
    const long b = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double gwb = 0.0, gdt = 0.0;
    if (w && !(mode && mode[b] != 0)) {
        const mpcqp_kin_vehicle& k = constants(ks, b);
        const double v = x[b * x_sb + 2], yaw = x[b * x_sb + 3], st = u[b * u_sb + 0], acc = u[b * u_sb + 1];
        const double dt = k.dt, wb = k.l_f + k.l_r;
        const double v1 = v + acc * dt;
        const double cy = cos(yaw), sy = sin(yaw), ts = tan(st);
        const double w0 = w[b * 4 + 0], w1 = w[b * 4 + 1], w2 = w[b * 4 + 2], w3 = w[b * 4 + 3];
        gwb = -(w3 * v1 * ts * dt) / (wb * wb);
        gdt = (v * (w0 * cy + w1 * sy) + w2 * acc) + w3 * ts * (acc * dt + v1) / wb;
    }
    gK[b * 3 + 0] = gwb;
    gK[b * 3 + 1] = gwb;
    gK[b * 3 + 2] = gdt;
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

// ---- F1 for the LTI (lateral) layouts: affine vector assembly ----
// vehicle_lateral_mpc_slack_increment.py:32-121 / its loop :201-229 and
// Control/MPC/mpc_kinematics.py:148-191 rebuild P, q, A, l, u every step although with the
// fixed lateral model only q (from xr), the initial-state rows of l = u (from x0) and the
// bound regime's inequality rows change.  Every entry of the concatenated (q, l, u) is an
// affine function of the instance's parameters theta = (x0, xr), with a base vector per
// bound regime:  v_i = base[regime][i] + sum_t coef[i][t] theta[idx[i][t]].  One thread per
// (instance, entry), consecutive threads on consecutive entries (coalesced stores).
struct AffineK {
    int L, R, T, seg0, seg1;  // entries, regimes, terms per entry, segment starts (q | l | u)
    const double *base, *coef;
    const int* idx;
};

__global__ __launch_bounds__(256) void k_affine(AffineK a, long B, const double* __restrict__ theta, int tstride,
                                                const int* __restrict__ regime, double* __restrict__ o0,
                                                double* __restrict__ o1, double* __restrict__ o2) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;
    if (g >= B * a.L) return;
    const long b = g / a.L;
    const int i = (int)(g - b * a.L);
    int r = regime ? regime[b] : 0;
    r = r < 0 ? 0 : (r >= a.R ? a.R - 1 : r);
    const double bv = a.base[(long)r * a.L + i];
    // the terms first, the base added only where it is nonzero: an entry the builder forms
    // as a product alone (q = -Q xr, l = u = -x0) is that product, bit for bit
    double v = 0.0;
    bool any = false;
    for (int t = 0; t < a.T; ++t) {
        const int k = a.idx[i * a.T + t];
        if (k >= 0) {
            const double term = a.coef[i * a.T + t] * theta[b * tstride + k];
            v = any ? v + term : term;
            any = true;
        }
    }
    v = !any ? bv : (bv != 0.0 ? bv + v : v);
    if (i < a.seg0) o0[b * a.seg0 + i] = v;
    else if (i < a.seg1) o1[b * (a.seg1 - a.seg0) + (i - a.seg0)] = v;
    else o2[b * (a.L - a.seg1) + (i - a.seg1)] = v;
}

// Transpose of k_affine's linear part: gtheta[b][p] = sum of coef[i][t] g[i] over the terms with
// idx[i][t] == p, in the order of the by-parameter lists (entry, then term).  One thread per
// (instance, parameter); a null cotangent segment reads as zero.
struct AffineVjpK {
    int L, seg0, seg1, nparam;
    const int *pptr, *pent;
    const double* pcoef;
};

__global__ __launch_bounds__(256) void k_affine_vjp(AffineVjpK a, long B, const double* __restrict__ g0,
                                                    const double* __restrict__ g1, const double* __restrict__ g2,
                                                    double* __restrict__ gtheta, long gstride) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= B * a.nparam) return;
    const long b = t / a.nparam;
    const int p = (int)(t - b * a.nparam);
    double v = 0.0;
    bool any = false;
    for (int s = a.pptr[p]; s < a.pptr[p + 1]; ++s) {
        const int i = a.pent[s];
        double g;
        if (i < a.seg0) g = g0 ? g0[b * a.seg0 + i] : 0.0;
        else if (i < a.seg1) g = g1 ? g1[b * (a.seg1 - a.seg0) + (i - a.seg0)] : 0.0;
        else g = g2 ? g2[b * (a.L - a.seg1) + (i - a.seg1)] : 0.0;
        const double term = a.pcoef[s] * g;
        v = any ? v + term : term;
        any = true;
    }
    gtheta[b * gstride + p] = v;
}

}  // namespace mpcqp

using namespace mpcqp;

struct mpcqp_incr_layout : IncrLayout {};
struct mpcqp_ltv_layout : IncrLayout {};  // nxa = nx: no augmentation

struct mpcqp_affine {
    int dev = 0, L = 0, R = 0, T = 0, seg0 = 0, seg1 = 0, nparam = 0;
    double *d_base = nullptr, *d_coef = nullptr;
    int* d_idx = nullptr;
    // the terms by parameter (for the VJP): parameter p's are pent / pcoef[pptr[p] .. pptr[p+1])
    int *d_pptr = nullptr, *d_pent = nullptr;
    double* d_pcoef = nullptr;
};

// A fleet: the B structs as given, each vehicle's constants (vehicle_constants, on the host, at
// creation) and their device table, uploaded by the first call that needs it.
template <class V, class KT>
struct Fleet {
    using Vehicle = V;
    using K = KT;
    int dev = 0;
    std::vector<V> veh;
    std::vector<KT> k;
    KT* d_k = nullptr;
};
struct mpcqp_fleet : Fleet<mpcqp_vehicle, VehicleK> {};
struct mpcqp_kin_fleet : Fleet<mpcqp_kin_vehicle, mpcqp_kin_vehicle> {};

namespace {

#define MHIPCHK(expr)                                                                        \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return set_error(MPCQP_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

template <class T>
int upload(const std::vector<T>& v, T** d) {
    MHIPCHK(hipMalloc((void**)d, sizeof(T) * std::max<size_t>(v.size(), 1)));
    if (!v.empty()) MHIPCHK(hipMemcpy(*d, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice));
    return 0;
}

int ensure_device(IncrLayout& L) {
    if (L.d_asrc) return 0;
    MHIPCHK(hipSetDevice(L.dev));
    if (int e = upload(L.asrc, &L.d_asrc)) return e;
    if (int e = upload(L.Atpl, &L.d_Atpl)) return e;
    if (int e = upload(L.ltpl, &L.d_ltpl)) return e;
    if (int e = upload(L.utpl, &L.d_utpl)) return e;
    if (int e = upload(L.Qt, &L.d_Qt)) return e;
    return 0;
}

// the reverse maps, the caller's weights and the per-call Qt scratch (VJP, *_assemble_w)
int ensure_reverse(IncrLayout& L) {
    if (L.d_Qtw) return 0;
    MHIPCHK(hipSetDevice(L.dev));
    if (int e = upload(L.adst, &L.d_adst)) return e;
    if (int e = upload(L.bdst, &L.d_bdst)) return e;
    if (int e = upload(L.psrc, &L.d_psrc)) return e;
    if (int e = upload(L.wptr, &L.d_wptr)) return e;
    if (int e = upload(L.wlist, &L.d_wlist)) return e;
    if (int e = upload(L.W, &L.d_W)) return e;
    if (int e = upload(L.Qt, &L.d_Qtw)) return e;
    return 0;
}

IncrK incr_k(const IncrLayout& L) {
    IncrK k;
    k.N = L.N; k.nx = L.nx; k.nu = L.nu; k.nxa = L.nxa; k.n = L.n; k.m = L.m; k.nnzA = (int)L.Ai.size();
    k.asrc = L.d_asrc; k.Atpl = L.d_Atpl; k.ltpl = L.d_ltpl; k.utpl = L.d_utpl; k.Qt = L.d_Qt;
    return k;
}

// P = blockdiag(kron(I_N, C'QC), C'QN C, kron(I_N, R)), upper triangle, zeros dropped
// (mpc_dynamics.py:304-307); with nxa = nx, C = I: blockdiag(Q x N, QN, R x N)
void build_P(IncrLayout& L, const double* Q, const double* QN, const double* R) {
    const int N = L.N, nx = L.nx, nu = L.nu, nxa = L.nxa, n = L.n, nq = nx * nx;
    L.Pp.assign(n + 1, 0);
    for (int c = 0; c < n; ++c) {
        if (c < (N + 1) * nxa) {
            const int k = c / nxa, j = c % nxa;
            const double* W = k == N ? QN : Q;
            if (j < nx)
                for (int i = 0; i <= j; ++i) {
                    const double v = W[i * nx + j];
                    if (v != 0.0) {
                        L.Pi.push_back(k * nxa + i); L.Px.push_back(v);
                        L.psrc.push_back((k == N ? nq : 0) + i * nx + j);
                    }
                }
        } else {
            const int c0 = c - (N + 1) * nxa, k = c0 / nu, j = c0 % nu;
            for (int i = 0; i <= j; ++i) {
                const double v = R[i * nu + j];
                if (v != 0.0) {
                    L.Pi.push_back((N + 1) * nxa + k * nu + i); L.Px.push_back(v);
                    L.psrc.push_back(2 * nq + i * nu + j);
                }
            }
        }
        L.Pp[c + 1] = (int)L.Pi.size();
    }
    // W and, per entry of it, the slots of P that hold it (ascending: stage order)
    L.W.assign(Q, Q + nq);
    L.W.insert(L.W.end(), QN, QN + nq);
    L.W.insert(L.W.end(), R, R + nu * nu);
    const int nw = (int)L.W.size();
    L.wptr.assign(nw + 1, 0);
    for (int s : L.psrc) L.wptr[s + 1] += 1;
    for (int w = 0; w < nw; ++w) L.wptr[w + 1] += L.wptr[w];
    L.wlist.assign(L.psrc.size(), 0);
    std::vector<int> fill(L.wptr.begin(), L.wptr.end() - 1);
    for (int e = 0; e < (int)L.psrc.size(); ++e) L.wlist[fill[L.psrc[e]]++] = e;
}

// dims / pattern / free of either layout (mpcqp_incr_layout, mpcqp_ltv_layout)
int layout_dims(const IncrLayout* L, const char* what, int32_t* n, int32_t* m, int32_t* nnzP, int32_t* nnzA) {
    if (!L || !n || !m || !nnzP || !nnzA) return set_error(MPCQP_EINVAL, "%s: NULL argument", what);
    *n = L->n; *m = L->m; *nnzP = (int32_t)L->Pi.size(); *nnzA = (int32_t)L->Ai.size();
    return 0;
}

int layout_pattern(const IncrLayout* L, const char* what, int32_t* Pp, int32_t* Pi, double* Px, int32_t* Ap,
                   int32_t* Ai, double* Ax_template, double* l_template, double* u_template) {
    if (!L) return set_error(MPCQP_EINVAL, "%s: NULL layout", what);
    if (Pp) std::memcpy(Pp, L->Pp.data(), sizeof(int32_t) * L->Pp.size());
    if (Pi) std::memcpy(Pi, L->Pi.data(), sizeof(int32_t) * L->Pi.size());
    if (Px) std::memcpy(Px, L->Px.data(), sizeof(double) * L->Px.size());
    if (Ap) std::memcpy(Ap, L->Ap.data(), sizeof(int32_t) * L->Ap.size());
    if (Ai) std::memcpy(Ai, L->Ai.data(), sizeof(int32_t) * L->Ai.size());
    if (Ax_template) std::memcpy(Ax_template, L->Atpl.data(), sizeof(double) * L->Atpl.size());
    if (l_template) std::memcpy(l_template, L->ltpl.data(), sizeof(double) * L->ltpl.size());
    if (u_template) std::memcpy(u_template, L->utpl.data(), sizeof(double) * L->utpl.size());
    return 0;
}

void layout_free_device(IncrLayout* L) {
    if (L->d_asrc) (void)hipSetDevice(L->dev);
    if (!L->d_asrc && L->d_Qtw) (void)hipSetDevice(L->dev);
    for (void* p : {(void*)L->d_asrc, (void*)L->d_Atpl, (void*)L->d_ltpl, (void*)L->d_utpl, (void*)L->d_Qt,
                    (void*)L->d_adst, (void*)L->d_bdst, (void*)L->d_psrc, (void*)L->d_wptr, (void*)L->d_wlist,
                    (void*)L->d_W, (void*)L->d_Qtw})
        if (p) (void)hipFree(p);
}

// P, the A pattern with its source codes, and Qt of a layout with nxa >= nx state columns per
// stage (:336-369, :381-382; mpc_kinematics_pred_matrix.py:293-309, :326, :341 for nxa = nx).
// The bounds (set_box) are the caller's.
void build_layout(IncrLayout& L, int N, int nx, int nu, int nxa, int device, const double* Q, const double* QN,
                  const double* R, const uint8_t* maskA, const uint8_t* maskB, bool transpose_Q) {
    const int ns = (N + 1) * nxa, n = ns + N * nu, m = ns + n;
    L.N = N; L.nx = nx; L.nu = nu; L.nxa = nxa; L.n = n; L.m = m; L.dev = device;
    build_P(L, Q, QN, R);
    L.Ap.assign(n + 1, 0);
    auto push = [&](int row, int src, double tpl) {
        L.Ai.push_back(row); L.asrc.push_back(src); L.Atpl.push_back(tpl);
    };
    for (int c = 0; c < n; ++c) {
        if (c < ns) {
            const int k = c / nxa, j = c % nxa;
            push(c, kConstSrc, -1.0);  // -I
            if (k < N)                 // A~_k in rows of stage k+1
                for (int i = 0; i < nxa; ++i) {
                    const int row = (k + 1) * nxa + i;
                    if (i < nx && j < nx) {
                        if (maskA[i * nx + j]) push(row, k * nx * nx + i * nx + j, 0.0);
                    } else if (i < nx) {
                        if (maskB[i * nu + (j - nx)]) push(row, -1 - (k * nx * nu + i * nu + (j - nx)), 0.0);
                    } else if (i == j) {
                        push(row, kConstSrc, 1.0);
                    }
                }
        } else {
            const int c0 = c - ns, k = c0 / nu, j = c0 % nu;  // du_k / u_k: B~_k in rows of stage k+1
            for (int i = 0; i < nxa; ++i) {
                const int row = (k + 1) * nxa + i;
                if (i < nx) {
                    if (maskB[i * nu + j]) push(row, -1 - (k * nx * nu + i * nu + j), 0.0);
                } else if (i - nx == j) {
                    push(row, kConstSrc, 1.0);
                }
            }
        }
        push(ns + c, kConstSrc, 1.0);  // A_ineq = I
        L.Ap[c + 1] = (int)L.Ai.size();
    }
    // where each stage entry went: asrc read backwards (slots ascend, so bdst's pair is in CSC order)
    L.adst.assign(N * nx * nx, -1);
    L.bdst.assign(2 * N * nx * nu, -1);
    for (int e = 0; e < (int)L.asrc.size(); ++e) {
        const int s = L.asrc[e];
        if (s == kConstSrc) continue;
        if (s >= 0) L.adst[s] = e;
        else {
            int* d = &L.bdst[2 * (-1 - s)];
            d[d[0] < 0 ? 0 : 1] = e;
        }
    }
    L.Qt.assign(2 * nx * nx, 0.0);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) {
            const int src = transpose_Q ? j * nx + i : i * nx + j;
            L.Qt[i * nx + j] = Q[src];
            L.Qt[nx * nx + i * nx + j] = QN[src];
        }
}

// Inequality-row bounds: xlo / xhi (nxa long) in every stage, ulo / uhi in every input stage,
// each through the caller's clipping (the osqp wrapper clips +-inf to +-OSQP_INFTY); equality rows 0.
constexpr double kInf = 1e30;
template <class ClipLo, class ClipHi>
void set_box(IncrLayout& L, const double* xlo, const double* xhi, const double* ulo, const double* uhi,
             ClipLo clip_lo, ClipHi clip_hi) {
    const int N = L.N, nu = L.nu, nxa = L.nxa, ns = (N + 1) * nxa;
    L.ltpl.assign(L.m, 0.0); L.utpl.assign(L.m, 0.0);
    for (int k = 0; k <= N; ++k)
        for (int i = 0; i < nxa; ++i) {
            L.ltpl[ns + k * nxa + i] = clip_lo(xlo[i]);
            L.utpl[ns + k * nxa + i] = clip_hi(xhi[i]);
        }
    for (int k = 0; k < N; ++k)
        for (int j = 0; j < nu; ++j) {
            L.ltpl[2 * ns + k * nu + j] = clip_lo(ulo[j]);
            L.utpl[2 * ns + k * nu + j] = clip_hi(uhi[j]);
        }
}

unsigned grid_of(long count, int block) { return (unsigned)((count + block - 1) / block); }

// hipSetDevice, one launch of `count` threads in blocks of `block`, hipGetLastError
template <class... P, class... A>
int launch(int device, void* stream, long count, int block, void (*kernel)(P...), A... args) {
    MHIPCHK(hipSetDevice(device));
    hipLaunchKernelGGL(kernel, dim3(grid_of(count, block)), dim3(block), 0, (hipStream_t)stream, (P)args...);
    MHIPCHK(hipGetLastError());
    return 0;
}

// The constants' source of a call, V: a vehicle struct (one car for the batch, by value) or a fleet
// (its table, entry b for vehicle b).  Every host function below that takes one is written once
// over V: source_check after its own argument checks and before any device call, then launch_from.
template <class V>
constexpr bool kIsFleet = std::is_same<V, mpcqp_fleet>::value || std::is_same<V, mpcqp_kin_fleet>::value;

// a fleet serves batches of its own size on its own device; a vehicle struct any
template <class V>
int source_check(const char* what, const V* veh, int64_t B, int device) {
    if constexpr (kIsFleet<V>) {
        if ((int64_t)veh->k.size() != B)
            return set_error(MPCQP_EINVAL, "%s: B = %lld is not the fleet's size %lld", what, (long long)B,
                             (long long)veh->k.size());
        if (veh->dev != device)
            return set_error(MPCQP_EINVAL, "%s: the fleet was created for device %d, the call is on device %d", what,
                             veh->dev, device);
    }
    return 0;
}

// launch(): `uniform` with the struct's constants, or `table` with the fleet's device table
// (uploaded here on first use), first among the kernel's arguments
#define BOTH_FORMS(kernel, K) kernel<K>, kernel<TableK<K>>  // `uniform`, `table` of a kernel template over KS
template <class V, class KU, class KT, class... A>
int launch_from(const V* veh, int device, void* stream, long count, int block, KU uniform, KT table, A... args) {
    if constexpr (kIsFleet<V>) {
        V& f = *const_cast<V*>(veh);
        if (!f.d_k) {
            MHIPCHK(hipSetDevice(f.dev));
            if (int e = upload(f.k, &f.d_k)) return e;
        }
        return launch(device, stream, count, block, table, TableK<typename V::K>{f.d_k}, args...);
    } else {
        return launch(device, stream, count, block, uniform, vehicle_constants(*veh), args...);
    }
}

template <class M, class V>
int linearise_device(const char* what, const V* veh, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                     int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, double* dAd, double* dBd,
                     double* dgd, int32_t device, void* stream) {
    if (!veh || !dx || !du || !dAd || !dBd || !dgd || B < 0 || N < 1)
        return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (int e = source_check(what, veh, B, device)) return e;
    if (B == 0) return 0;
    return launch_from(veh, device, stream, B * N, 256, k_linearise<M>, k_linearise<OverFleet<M>>, B, N, dx, x_sb,
                       x_sk, du, u_sb, u_sk, dAd, dBd, dgd);
}

// M: the model, which selects the kernel pair (the dynamic bicycle's duals, the kinematic closed form)
template <class M, class V>
int linearise_vjp_device(const char* what, const V* veh, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                         int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, const double* dgAd,
                         const double* dgBd, const double* dggd, double* dgx, double* dgu, int32_t device,
                         void* stream) {
    if (!veh || !dx || !du || B < 0 || N < 1) return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (int e = source_check(what, veh, B, device)) return e;
    if (B == 0 || (!dgx && !dgu)) return 0;
    if constexpr (M::NX == 6)
        return launch_from(veh, device, stream, B * N, 256, BOTH_FORMS(k_linearise_vjp, VehicleK), B, N, dx, x_sb,
                           x_sk, du, u_sb, u_sk, dgAd, dgBd, dggd, dgx, dgu);
    else
        return launch_from(veh, device, stream, B * N, 256, BOTH_FORMS(k_kin_linearise_vjp, mpcqp_kin_vehicle), B, N, dx,
                           x_sb, x_sk, du, u_sb, u_sk, dgAd, dgBd, dggd, dgx, dgu);
}

// The parameter kernels exist in fleet form only; the fleet's table, uploaded on
// first use as launch_from does.
template <class F>
int fleet_table(const F* fleet, TableK<typename F::K>* out) {
    F& f = *const_cast<F*>(fleet);
    if (!f.d_k) {
        MHIPCHK(hipSetDevice(f.dev));
        if (int e = upload(f.k, &f.d_k)) return e;
    }
    out->k = f.d_k;
    return 0;
}

constexpr int kStageSumMax = 256;  // one block holds whole vehicles: N stages of one fit 256 threads

// F: mpcqp_fleet (gK (B, 13), two launches, one per group of constants) or mpcqp_kin_fleet ((B, 3))
template <class F>
int linearise_pvjp_device(const char* what, const F* f, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                          int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, const double* dgAd,
                          const double* dgBd, const double* dggd, double* dgK, int32_t device, void* stream) {
    if (!f || !dx || !du || !dgK || B < 0 || N < 1) return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (N > kStageSumMax)
        return set_error(MPCQP_EUNSUPPORTED, "%s: need N <= %d (the stage sum holds whole vehicles in one block)",
                         what, kStageSumMax);
    if (int e = source_check(what, f, B, device)) return e;
    if (B == 0) return 0;
    TableK<typename F::K> table;
    if (int e = fleet_table(f, &table)) return e;
    const int vpb = kStageSumMax / N;
    const long threads = (long)grid_of(B, vpb) * 256;
    if constexpr (std::is_same<F, mpcqp_fleet>::value) {
        if (int e = launch(device, stream, threads, 256, k_linearise_pvjp<0, 7>, table, B, N, vpb, dx, x_sb, x_sk,
                           du, u_sb, u_sk, dgAd, dgBd, dggd, dgK))
            return e;
        return launch(device, stream, threads, 256, k_linearise_pvjp<7, 6>, table, B, N, vpb, dx, x_sb, x_sk, du,
                      u_sb, u_sk, dgAd, dgBd, dggd, dgK);
    } else {
        return launch(device, stream, threads, 256, k_kin_linearise_pvjp, table, B, N, vpb, dx, x_sb, x_sk, du, u_sb,
                      u_sk, dgAd, dgBd, dggd, dgK);
    }
}

// the terminal step of a tail with respect to the constants: euler_step_guarded / kin_update
template <class F>
int step_pvjp_device(const char* what, const F* f, int64_t B, const double* dx, int64_t x_sb, const double* du,
                     int64_t u_sb, const double* dw, const int32_t* dmode, double* dgK, int32_t device,
                     void* stream) {
    if (!f || !dx || !du || !dgK || B < 0) return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (int e = source_check(what, f, B, device)) return e;
    if (B == 0) return 0;
    TableK<typename F::K> table;
    if (int e = fleet_table(f, &table)) return e;
    if constexpr (std::is_same<F, mpcqp_fleet>::value)
        return launch(device, stream, B, 128, k_euler_step_pvjp, table, B, dx, x_sb, du, u_sb, dw, dmode, dgK);
    else
        return launch(device, stream, B, 128, k_kin_update_pvjp, table, B, dx, x_sb, du, u_sb, dw, dmode, dgK);
}

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

// mpcqp_fleet_create / mpcqp_kin_fleet_create: the refusals, then every vehicle's constants
inline const double* fields_of(const mpcqp_vehicle& v, int* n) { *n = 9; return &v.m; }
inline const double* fields_of(const mpcqp_kin_vehicle& v, int* n) { *n = 3; return &v.l_f; }
inline bool inertia_ok(const mpcqp_vehicle& v) { return v.m > 0.0 && v.width * v.width + v.length * v.length != 0.0; }
inline bool inertia_ok(const mpcqp_kin_vehicle&) { return true; }  // the kinematic model has none

template <class F, class V>
int fleet_create(int64_t B, const V* veh, int32_t device, F** out) {
    if (!veh || !out) return set_error(MPCQP_EINVAL, "fleet_create: NULL argument");
    *out = nullptr;
    if (B < 1) return set_error(MPCQP_EINVAL, "fleet_create: need B >= 1");
    for (int64_t b = 0; b < B; ++b) {
        int nf = 0;
        const double* f = fields_of(veh[b], &nf);
        for (int i = 0; i < nf; ++i)
            if (!std::isfinite(f[i]))
                return set_error(MPCQP_EINVAL, "fleet_create: vehicle %lld has a non-finite field", (long long)b);
        if (!(veh[b].l_f > 0.0) || !(veh[b].l_r > 0.0) || !(veh[b].dt > 0.0) || !inertia_ok(veh[b]))
            return set_error(MPCQP_EINVAL,
                             "fleet_create: vehicle %lld needs m, l_f, l_r, dt > 0 and width^2 + length^2 > 0",
                             (long long)b);
        if (veh[b].dt != veh[0].dt)
            return set_error(MPCQP_EINVAL, "fleet_create: vehicle %lld has dt %.17g, vehicle 0 has %.17g: one dt per fleet",
                             (long long)b, veh[b].dt, veh[0].dt);
    }
    auto f = std::make_unique<F>();
    f->dev = device;
    f->veh.assign(veh, veh + B);
    f->k.reserve(B);
    for (int64_t b = 0; b < B; ++b) f->k.push_back(vehicle_constants(veh[b]));
    *out = f.release();  // the table is uploaded by the first device call that takes the fleet
    return 0;
}

template <class F>
void fleet_free(F* f) {
    if (!f) return;
    if (f->d_k) {
        (void)hipSetDevice(f->dev);
        (void)hipFree(f->d_k);
    }
    delete f;
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

// dxlo, dxhi: per-stage state bounds (B, N+1, nxa), either may be null
int assemble_device(const char* what, const IncrLayout* L, int64_t B, const double* dAd, const double* dBd,
                    const double* dgd, const double* dx0, const double* dXr, const double* dxlo, const double* dxhi,
                    double* dAx, double* dq, double* dl, double* du, void* stream) {
    if (!L || !dAd || !dBd || !dgd || !dx0 || !dXr || !dAx || !dq || !dl || !du || B < 0)
        return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (B == 0) return 0;
    if (int e = ensure_device(*const_cast<IncrLayout*>(L))) return e;
    const IncrK k = incr_k(*L);
    if (int e = launch(L->dev, stream, B * k.nnzA, 256, k_incr_assemble_A, k, B, dAd, dBd, dAx)) return e;
    return launch(L->dev, stream, B, 128, k_incr_assemble_vec, k, B, dgd, dx0, dXr, dxlo, dxhi, dq, dl, du);
}

// assemble_device with the weights of this call (each null: the layout's own): k_weights writes
// the Qt scratch and dPx, then the forward kernels run unchanged with IncrK::Qt on the scratch
int assemble_w_device(const char* what, const IncrLayout* L, int64_t B, const double* dAd, const double* dBd,
                      const double* dgd, const double* dx0, const double* dXr, const double* dxlo, const double* dxhi,
                      const double* dQ, const double* dQN, const double* dR, double* dAx, double* dq, double* dl,
                      double* du, double* dPx, void* stream) {
    if (!L || !dAd || !dBd || !dgd || !dx0 || !dXr || !dAx || !dq || !dl || !du || B < 0)
        return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (B == 0) return 0;
    IncrLayout& M = *const_cast<IncrLayout*>(L);
    if (int e = ensure_device(M)) return e;
    if (int e = ensure_reverse(M)) return e;
    const int nq = L->nx * L->nx, nnzP = (int)L->Pi.size();
    if (int e = launch(L->dev, stream, 2 * nq + nnzP, 256, k_weights, L->nx, nnzP, (int)(L->nxa != L->nx), L->d_psrc,
                       dQ ? dQ : L->d_W, dQN ? dQN : L->d_W + nq, dR ? dR : L->d_W + 2 * nq, L->d_Qtw, dPx))
        return e;
    IncrK k = incr_k(*L);
    k.Qt = L->d_Qtw;
    if (int e = launch(L->dev, stream, B * k.nnzA, 256, k_incr_assemble_A, k, B, dAd, dBd, dAx)) return e;
    return launch(L->dev, stream, B, 128, k_incr_assemble_vec, k, B, dgd, dx0, dXr, dxlo, dxhi, dq, dl, du);
}

// The transpose of assemble_device (and of assemble_w_device: dQ / dQN the weights that call took,
// null the layout's own).  Every cotangent and every output may be null.
int assemble_vjp_device(const char* what, const IncrLayout* L, int64_t B, const double* dgPx, const double* dgAx,
                        const double* dgq, const double* dgl, const double* dgu, const double* dXr,
                        const double* dxlo, const double* dxhi, const double* dQ, const double* dQN, double* dgAd,
                        double* dgBd, double* dggd, double* dgx0, double* dgXr, double* dgxlo, double* dgxhi,
                        double* dgQ, double* dgQN, double* dgR, void* stream) {
    if (!L) return set_error(MPCQP_EINVAL, "%s: NULL layout", what);
    if (B < 0) return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if ((dgxlo && !dxlo) || (dgxhi && !dxhi))
        return set_error(MPCQP_EINVAL, "%s: gxlo / gxhi need the forward call's xlo / xhi", what);
    if ((dgQ || dgQN) && dgq && !dXr)
        return set_error(MPCQP_EINVAL, "%s: gQ / gQN from gq need the forward call's Xr", what);
    if (B == 0) return 0;
    IncrLayout& M = *const_cast<IncrLayout*>(L);
    if (int e = ensure_device(M)) return e;
    if (int e = ensure_reverse(M)) return e;
    const int N = L->N, nx = L->nx, nu = L->nu, nxa = L->nxa, nq = nx * nx;
    VjpK k;
    k.N = N; k.nx = nx; k.nu = nu; k.nxa = nxa; k.n = L->n; k.m = L->m;
    k.nnzA = (int)L->Ai.size(); k.nnzP = (int)L->Pi.size();
    k.adst = L->d_adst; k.bdst = L->d_bdst; k.wptr = L->d_wptr; k.wlist = L->d_wlist;
    // the forward's W_k[i][j]: the layout's Qt as it stands, or the caller's Q read transposed
    // under the augmented layout
    k.tr = 0; k.Wst = L->d_Qt; k.Wtm = L->d_Qt + nq;
    if (dQ || dQN) {
        k.tr = nxa != nx;
        k.Wst = dQ ? dQ : L->d_W;
        k.Wtm = dQN ? dQN : L->d_W + nq;
    }
    if (dgAd || dgBd)
        if (int e = launch(L->dev, stream, B * N * (nq + nx * nu), 256, k_assemble_vjp_AB, k, B, dgAx, dgAd, dgBd))
            return e;
    if (dggd || dgx0 || dgXr || dgxlo || dgxhi) {
        const long per = (long)N * nx + nxa + (long)nx * (N + 1) + 2L * (N + 1) * nxa;
        if (int e = launch(L->dev, stream, B * per, 256, k_assemble_vjp_vec, k, B, dgq, dgl, dgu, dxlo, dxhi, dggd,
                           dgx0, dgXr, dgxlo, dgxhi))
            return e;
    }
    if (dgQ || dgQN || dgR) {
        k.tr = nxa != nx;  // here the orientation is the caller's Q's, whatever W the forward read
        if (int e = launch(L->dev, stream, B * (2 * nq + nu * nu), 256, k_assemble_vjp_w, k, B, dgPx, dgq, dXr, dgQ,
                           dgQN, dgR))
            return e;
    }
    return 0;
}

}  // namespace

extern "C" {

int mpcqp_linearise_device(const mpcqp_vehicle* veh, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                           int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, double* dAd, double* dBd,
                           double* dgd, int32_t device, void* stream) {
    return linearise_device<DynamicBicycle>("linearise", veh, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dAd, dBd, dgd,
                                            device, stream);
}

int mpcqp_kin_linearise_device(const mpcqp_kin_vehicle* veh, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                               int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, double* dAd, double* dBd,
                               double* dgd, int32_t device, void* stream) {
    return linearise_device<KinematicBicycle>("kin_linearise", veh, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dAd, dBd,
                                              dgd, device, stream);
}

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

int mpcqp_incr_layout_create(int32_t N, int32_t nx, int32_t nu, const double* Q, const double* QN, const double* R,
                             const double* xmin_t, const double* xmax_t, const double* dumin, const double* dumax,
                             const uint8_t* maskA, const uint8_t* maskB, int32_t device, mpcqp_incr_layout** out) {
    if (!out || !Q || !QN || !R || !xmin_t || !xmax_t || !dumin || !dumax || !maskA || !maskB)
        return set_error(MPCQP_EINVAL, "incr_layout_create: NULL argument");
    if (N < 2 || nx < 1 || nu < 1 || nx > 6 || nu > 2)
        return set_error(MPCQP_EUNSUPPORTED, "incr_layout_create: need N >= 2, 1 <= nx <= 6, 1 <= nu <= 2");
    for (int i = 0; i < nx + nu; ++i)
        if (!(xmin_t[i] <= xmax_t[i])) return set_error(MPCQP_EINVAL, "incr_layout_create: xmin_t > xmax_t");
    for (int j = 0; j < nu; ++j)
        if (!(dumin[j] <= dumax[j])) return set_error(MPCQP_EINVAL, "incr_layout_create: dumin > dumax");
    *out = nullptr;
    auto L = std::make_unique<mpcqp_incr_layout>();
    // (Q C)' restricted to its nx x nx nonzero block: Q transposed
    build_layout(*L, N, nx, nu, nx + nu, device, Q, QN, R, maskA, maskB, true);
    // inequality bounds (:383-384): lower bounds clipped from below, upper from above
    set_box(*L, xmin_t, xmax_t, dumin, dumax, [](double v) { return std::max(v, -kInf); },
            [](double v) { return std::min(v, kInf); });
    *out = L.release();  // device copies are made by the first assemble / shift (host-only use needs no GPU)
    return 0;
}

int mpcqp_ltv_layout_create(int32_t N, int32_t nx, int32_t nu, const double* Q, const double* QN, const double* R,
                            const double* xmin, const double* xmax, const double* umin, const double* umax,
                            const uint8_t* maskA, const uint8_t* maskB, int32_t device, mpcqp_ltv_layout** out) {
    if (!out || !Q || !QN || !R || !xmin || !xmax || !umin || !umax || !maskA || !maskB)
        return set_error(MPCQP_EINVAL, "ltv_layout_create: NULL argument");
    if (N < 2 || nx < 1 || nu < 1 || nx > 6 || nu > 2)
        return set_error(MPCQP_EUNSUPPORTED, "ltv_layout_create: need N >= 2, 1 <= nx <= 6, 1 <= nu <= 2");
    for (int i = 0; i < nx; ++i)
        if (!(xmin[i] <= xmax[i])) return set_error(MPCQP_EINVAL, "ltv_layout_create: xmin > xmax");
    for (int j = 0; j < nu; ++j)
        if (!(umin[j] <= umax[j])) return set_error(MPCQP_EINVAL, "ltv_layout_create: umin > umax");
    *out = nullptr;
    auto L = std::make_unique<mpcqp_ltv_layout>();
    // q = -Q Xr_k: the weights themselves
    build_layout(*L, N, nx, nu, nx, device, Q, QN, R, maskA, maskB, false);
    // box bounds (:327-328): every bound clipped on both sides
    const auto clip = [](double v) { return std::min(std::max(v, -kInf), kInf); };
    set_box(*L, xmin, xmax, umin, umax, clip, clip);
    *out = L.release();  // device copies are made by the first assemble (host-only use needs no GPU)
    return 0;
}

int mpcqp_incr_layout_dims(const mpcqp_incr_layout* L, int32_t* n, int32_t* m, int32_t* nnzP, int32_t* nnzA) {
    return layout_dims(L, "incr_layout_dims", n, m, nnzP, nnzA);
}

int mpcqp_ltv_layout_dims(const mpcqp_ltv_layout* L, int32_t* n, int32_t* m, int32_t* nnzP, int32_t* nnzA) {
    return layout_dims(L, "ltv_layout_dims", n, m, nnzP, nnzA);
}

int mpcqp_incr_layout_pattern(const mpcqp_incr_layout* L, int32_t* Pp, int32_t* Pi, double* Px, int32_t* Ap,
                              int32_t* Ai, double* Ax_template, double* l_template, double* u_template) {
    return layout_pattern(L, "incr_layout_pattern", Pp, Pi, Px, Ap, Ai, Ax_template, l_template, u_template);
}

int mpcqp_ltv_layout_pattern(const mpcqp_ltv_layout* L, int32_t* Pp, int32_t* Pi, double* Px, int32_t* Ap,
                             int32_t* Ai, double* Ax_template, double* l_template, double* u_template) {
    return layout_pattern(L, "ltv_layout_pattern", Pp, Pi, Px, Ap, Ai, Ax_template, l_template, u_template);
}

int mpcqp_incr_assemble_device(const mpcqp_incr_layout* L, int64_t B, const double* dAd, const double* dBd,
                               const double* dgd, const double* dxt0, const double* dXr, double* dAx, double* dq,
                               double* dl, double* du, void* stream) {
    return assemble_device("incr_assemble", L, B, dAd, dBd, dgd, dxt0, dXr, nullptr, nullptr, dAx, dq, dl, du, stream);
}

int mpcqp_ltv_assemble_device(const mpcqp_ltv_layout* L, int64_t B, const double* dAd, const double* dBd,
                              const double* dgd, const double* dx0, const double* dXr, const double* dxlo,
                              const double* dxhi, double* dAx, double* dq, double* dl, double* du, void* stream) {
    return assemble_device("ltv_assemble", L, B, dAd, dBd, dgd, dx0, dXr, dxlo, dxhi, dAx, dq, dl, du, stream);
}

int mpcqp_incr_assemble_w_device(const mpcqp_incr_layout* L, int64_t B, const double* dAd, const double* dBd,
                                 const double* dgd, const double* dxt0, const double* dXr, const double* dQ,
                                 const double* dQN, const double* dR, double* dAx, double* dq, double* dl, double* du,
                                 double* dPx, void* stream) {
    return assemble_w_device("incr_assemble_w", L, B, dAd, dBd, dgd, dxt0, dXr, nullptr, nullptr, dQ, dQN, dR, dAx, dq,
                             dl, du, dPx, stream);
}

int mpcqp_ltv_assemble_w_device(const mpcqp_ltv_layout* L, int64_t B, const double* dAd, const double* dBd,
                                const double* dgd, const double* dx0, const double* dXr, const double* dxlo,
                                const double* dxhi, const double* dQ, const double* dQN, const double* dR, double* dAx,
                                double* dq, double* dl, double* du, double* dPx, void* stream) {
    return assemble_w_device("ltv_assemble_w", L, B, dAd, dBd, dgd, dx0, dXr, dxlo, dxhi, dQ, dQN, dR, dAx, dq, dl, du,
                             dPx, stream);
}

int mpcqp_incr_assemble_vjp_device(const mpcqp_incr_layout* L, int64_t B, const double* dgPx, const double* dgAx,
                                   const double* dgq, const double* dgl, const double* dgu, const double* dXr,
                                   const double* dQ, const double* dQN, double* dgAd, double* dgBd, double* dggd,
                                   double* dgxt0, double* dgXr, double* dgQ, double* dgQN, double* dgR, void* stream) {
    return assemble_vjp_device("incr_assemble_vjp", L, B, dgPx, dgAx, dgq, dgl, dgu, dXr, nullptr, nullptr, dQ, dQN,
                               dgAd, dgBd, dggd, dgxt0, dgXr, nullptr, nullptr, dgQ, dgQN, dgR, stream);
}

int mpcqp_ltv_assemble_vjp_device(const mpcqp_ltv_layout* L, int64_t B, const double* dgPx, const double* dgAx,
                                  const double* dgq, const double* dgl, const double* dgu, const double* dXr,
                                  const double* dxlo, const double* dxhi, const double* dQ, const double* dQN,
                                  double* dgAd, double* dgBd, double* dggd, double* dgx0, double* dgXr, double* dgxlo,
                                  double* dgxhi, double* dgQ, double* dgQN, double* dgR, void* stream) {
    return assemble_vjp_device("ltv_assemble_vjp", L, B, dgPx, dgAx, dgq, dgl, dgu, dXr, dxlo, dxhi, dQ, dQN, dgAd,
                               dgBd, dggd, dgx0, dgXr, dgxlo, dgxhi, dgQ, dgQN, dgR, stream);
}

int mpcqp_kin_linearise_vjp_device(const mpcqp_kin_vehicle* veh, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                                   int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, const double* dgAd,
                                   const double* dgBd, const double* dggd, double* dgx, double* dgu, int32_t device,
                                   void* stream) {
    return linearise_vjp_device<KinematicBicycle>("kin_linearise_vjp", veh, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dgAd,
                                                  dgBd, dggd, dgx, dgu, device, stream);
}

int mpcqp_linearise_vjp_device(const mpcqp_vehicle* veh, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                               int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, const double* dgAd,
                               const double* dgBd, const double* dggd, double* dgx, double* dgu, int32_t device,
                               void* stream) {
    return linearise_vjp_device<DynamicBicycle>("linearise_vjp", veh, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dgAd, dgBd,
                                                dggd, dgx, dgu, device, stream);
}

void mpcqp_incr_layout_free(mpcqp_incr_layout* L) {
    if (!L) return;
    layout_free_device(L);
    delete L;
}

void mpcqp_ltv_layout_free(mpcqp_ltv_layout* L) {
    if (!L) return;
    layout_free_device(L);
    delete L;
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

int mpcqp_affine_create(int32_t nseg, const int32_t* seglen, int32_t nregimes, int32_t T, const double* base,
                        const int32_t* idx, const double* coef, int32_t device, mpcqp_affine** out) {
    if (!out || !seglen || !base || (T > 0 && (!idx || !coef)) || nseg < 1 || nseg > 3 || nregimes < 1 || T < 0)
        return set_error(MPCQP_EINVAL, "affine_create: bad arguments");
    *out = nullptr;
    auto a = std::make_unique<mpcqp_affine>();
    int L = 0, st[3] = {0, 0, 0};
    for (int s = 0; s < nseg; ++s) {
        if (seglen[s] < 0) return set_error(MPCQP_EINVAL, "affine_create: negative segment length");
        L += seglen[s];
        st[s] = L;
    }
    if (L == 0) return set_error(MPCQP_EINVAL, "affine_create: empty map");
    a->dev = device; a->L = L; a->R = nregimes; a->T = T;
    a->seg0 = st[0]; a->seg1 = nseg > 1 ? st[1] : L;
    if (nseg == 1) a->seg0 = a->seg1 = L;
    std::vector<double> vb(base, base + (size_t)nregimes * L), vc;
    std::vector<int> vi;
    if (T > 0) {
        vc.assign(coef, coef + (size_t)L * T);
        vi.assign(idx, idx + (size_t)L * T);
    } else {
        vc.assign(1, 0.0);
        vi.assign(1, -1);
    }
    for (int k : vi) a->nparam = std::max(a->nparam, k + 1);
    MHIPCHK(hipSetDevice(device));
    if (int e = upload(vb, &a->d_base)) return e;
    if (int e = upload(vc, &a->d_coef)) return e;
    if (int e = upload(vi, &a->d_idx)) return e;
    // the same terms listed by parameter, entries ascending and an entry's terms in their order
    std::vector<int> pptr(a->nparam + 1, 0), pent;
    std::vector<double> pcoef;
    for (int k : vi)
        if (k >= 0) pptr[k + 1] += 1;
    for (int p = 0; p < a->nparam; ++p) pptr[p + 1] += pptr[p];
    pent.assign(pptr[a->nparam], 0);
    pcoef.assign(pptr[a->nparam], 0.0);
    std::vector<int> fill(pptr.begin(), pptr.end() - 1);
    for (size_t s = 0; s < vi.size(); ++s)
        if (vi[s] >= 0) {
            const int at = fill[vi[s]]++;
            pent[at] = (int)(s / (size_t)std::max(T, 1));
            pcoef[at] = vc[s];
        }
    if (int e = upload(pptr, &a->d_pptr)) return e;
    if (int e = upload(pent, &a->d_pent)) return e;
    if (int e = upload(pcoef, &a->d_pcoef)) return e;
    *out = a.release();
    return 0;
}

int mpcqp_affine_vjp_device(const mpcqp_affine* a, int64_t B, const double* dg0, const double* dg1, const double* dg2,
                            const int32_t* dregime, double* dgtheta, int32_t gtheta_stride, void* stream) {
    if (!a) return set_error(MPCQP_EINVAL, "affine_vjp: NULL affine map");
    if (B < 0 || (dgtheta && gtheta_stride < a->nparam))
        return set_error(MPCQP_EINVAL, "affine_vjp: bad arguments (gtheta_stride must cover the %d parameters)",
                         a->nparam);
    (void)dregime;  // the regime selects the base, which has no derivative
    if (B == 0 || !dgtheta || a->nparam == 0) return 0;
    AffineVjpK k;
    k.L = a->L; k.seg0 = a->seg0; k.seg1 = a->seg1; k.nparam = a->nparam;
    k.pptr = a->d_pptr; k.pent = a->d_pent; k.pcoef = a->d_pcoef;
    return launch(a->dev, stream, B * a->nparam, 256, k_affine_vjp, k, B, dg0, dg1, dg2, dgtheta, gtheta_stride);
}

int mpcqp_affine_apply_device(const mpcqp_affine* a, int64_t B, const double* dtheta, int32_t theta_stride,
                              const int32_t* dregime, double* dout0, double* dout1, double* dout2, void* stream) {
    if (!a || B < 0 || (a->nparam > 0 && (!dtheta || theta_stride < a->nparam)) || !dout0 ||
        (a->seg1 > a->seg0 && !dout1) || (a->L > a->seg1 && !dout2))
        return set_error(MPCQP_EINVAL, "affine_apply: bad arguments (theta_stride must cover the %d parameters)",
                         a ? a->nparam : 0);
    if (B == 0) return 0;
    MHIPCHK(hipSetDevice(a->dev));
    AffineK k;
    k.L = a->L; k.R = a->R; k.T = a->T; k.seg0 = a->seg0; k.seg1 = a->seg1;
    k.base = a->d_base; k.coef = a->d_coef; k.idx = a->d_idx;
    if (a->T == 0) k.T = 0;
    hipLaunchKernelGGL(k_affine, dim3(grid_of((long)B * a->L, 256)), dim3(256), 0, (hipStream_t)stream, k, (long)B,
                       dtheta, (int)theta_stride, dregime, dout0, dout1, dout2);
    MHIPCHK(hipGetLastError());
    return 0;
}

void mpcqp_affine_free(mpcqp_affine* a) {
    if (!a) return;
    (void)hipSetDevice(a->dev);
    for (void* p : {(void*)a->d_base, (void*)a->d_coef, (void*)a->d_idx, (void*)a->d_pptr, (void*)a->d_pent,
                    (void*)a->d_pcoef})
        if (p) (void)hipFree(p);
    delete a;
}

// ---- fleets: one table of constants per batch, and the twin of every entry point above that
// takes a vehicle (the same host code over the constants' source) ----

int mpcqp_fleet_create(int64_t B, const mpcqp_vehicle* veh, int32_t device, mpcqp_fleet** out) {
    return fleet_create(B, veh, device, out);
}

int mpcqp_kin_fleet_create(int64_t B, const mpcqp_kin_vehicle* veh, int32_t device, mpcqp_kin_fleet** out) {
    return fleet_create(B, veh, device, out);
}

int mpcqp_fleet_constants(const mpcqp_fleet* f, int64_t b, double* out13) {
    if (!f || !out13) return set_error(MPCQP_EINVAL, "fleet_constants: NULL argument");
    if (b < 0 || b >= (int64_t)f->k.size())
        return set_error(MPCQP_EINVAL, "fleet_constants: vehicle %lld of a fleet of %lld", (long long)b,
                         (long long)f->k.size());
    static_assert(sizeof(VehicleK) == 13 * sizeof(double), "VehicleK is thirteen doubles");
    std::memcpy(out13, &f->k[b], sizeof(VehicleK));
    return 0;
}

void mpcqp_fleet_free(mpcqp_fleet* f) { fleet_free(f); }
void mpcqp_kin_fleet_free(mpcqp_kin_fleet* f) { fleet_free(f); }

int mpcqp_linearise_fleet_device(const mpcqp_fleet* f, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                                 int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, double* dAd, double* dBd,
                                 double* dgd, int32_t device, void* stream) {
    return linearise_device<DynamicBicycle>("linearise_fleet", f, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dAd, dBd, dgd,
                                            device, stream);
}

int mpcqp_kin_linearise_fleet_device(const mpcqp_kin_fleet* f, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                                     int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, double* dAd,
                                     double* dBd, double* dgd, int32_t device, void* stream) {
    return linearise_device<KinematicBicycle>("kin_linearise_fleet", f, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dAd, dBd,
                                              dgd, device, stream);
}

int mpcqp_linearise_vjp_fleet_device(const mpcqp_fleet* f, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                                     int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, const double* dgAd,
                                     const double* dgBd, const double* dggd, double* dgx, double* dgu, int32_t device,
                                     void* stream) {
    return linearise_vjp_device<DynamicBicycle>("linearise_vjp_fleet", f, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dgAd,
                                                dgBd, dggd, dgx, dgu, device, stream);
}

int mpcqp_kin_linearise_vjp_fleet_device(const mpcqp_kin_fleet* f, int64_t B, int32_t N, const double* dx,
                                         int64_t x_sb, int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk,
                                         const double* dgAd, const double* dgBd, const double* dggd, double* dgx,
                                         double* dgu, int32_t device, void* stream) {
    return linearise_vjp_device<KinematicBicycle>("kin_linearise_vjp_fleet", f, B, N, dx, x_sb, x_sk, du, u_sb, u_sk,
                                                  dgAd, dgBd, dggd, dgx, dgu, device, stream);
}

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

// ---- gradients with respect to a fleet's constants ----

int mpcqp_linearise_pvjp_fleet_device(const mpcqp_fleet* f, int64_t B, int32_t N, const double* dx, int64_t x_sb,
                                      int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk, const double* dgAd,
                                      const double* dgBd, const double* dggd, double* dgK, int32_t device,
                                      void* stream) {
    return linearise_pvjp_device("linearise_pvjp_fleet", f, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dgAd, dgBd, dggd,
                                 dgK, device, stream);
}

int mpcqp_kin_linearise_pvjp_fleet_device(const mpcqp_kin_fleet* f, int64_t B, int32_t N, const double* dx,
                                          int64_t x_sb, int64_t x_sk, const double* du, int64_t u_sb, int64_t u_sk,
                                          const double* dgAd, const double* dgBd, const double* dggd, double* dgK,
                                          int32_t device, void* stream) {
    return linearise_pvjp_device("kin_linearise_pvjp_fleet", f, B, N, dx, x_sb, x_sk, du, u_sb, u_sk, dgAd, dgBd,
                                 dggd, dgK, device, stream);
}

int mpcqp_euler_step_pvjp_fleet_device(const mpcqp_fleet* f, int64_t B, const double* dx, int64_t x_sb,
                                       const double* du, int64_t u_sb, const double* dw, const int32_t* dmode,
                                       double* dgK, int32_t device, void* stream) {
    return step_pvjp_device("euler_step_pvjp_fleet", f, B, dx, x_sb, du, u_sb, dw, dmode, dgK, device, stream);
}

int mpcqp_kin_update_pvjp_fleet_device(const mpcqp_kin_fleet* f, int64_t B, const double* dx, int64_t x_sb,
                                       const double* du, int64_t u_sb, const double* dw, const int32_t* dmode,
                                       double* dgK, int32_t device, void* stream) {
    return step_pvjp_device("kin_update_pvjp_fleet", f, B, dx, x_sb, du, u_sb, dw, dmode, dgK, device, stream);
}

int mpcqp_vehicle_constants_vjp(const mpcqp_vehicle* veh, const double gk[13], double gveh[9]) {
    if (!veh || !gk || !gveh) return set_error(MPCQP_EINVAL, "vehicle_constants_vjp: NULL argument");
    // derive_constants over duals in the nine arguments: d constant c / d argument a = k[c].d[a]
    using D9 = DualN<9>;
    D9 p[9], k[13];
    const double* v = &veh->m;
    for (int a = 0; a < 9; ++a) p[a] = D9(v[a], a, true);
    derive_constants(p, k);
    for (int a = 0; a < 9; ++a) {
        double acc = 0.0;
        for (int c = 0; c < 13; ++c) acc += gk[c] * k[c].d[a];
        gveh[a] = acc;
    }
    return 0;
}

}  // extern "C"
