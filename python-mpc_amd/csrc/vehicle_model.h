// vehicle_model.h -- the two vehicle models of the MPC data path and the dual numbers they are
// differentiated with; the only place the models are written.  Everything here is a template,
// __forceinline__, static or inline, so any number of files may include it:
//
//       VehicleK, derive_constants      constants of Vehicle_Dynamics          vehicle_models.py:27-50, :114-132
//       continuous_model                get_dynamics_model's f, Ac, Bc         vehicle_models.py:52-340
//       euler_step                      update_dynamics_model                  vehicle_models.py:343-477
//       kin_update                      update_kinematics_model                vehicle_models.py:866-883
// The two bicycles are model structs (DynamicBicycle, KinematicBicycle) over which the
// linearisation and the reference walk are written once.  The device functions built on these
// that are neither templates nor __forceinline__ (linearise_one, euler_step_guarded,
// euler_step_vjp) live in the one .hip file that calls them.  All fp64.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/mpcqp.h"

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
// A model or a Tail (mpc_device.hip) over a fleet: the kernels that are templates over one take M::K
// by value, so the table goes where the struct went; everything else of M is M's.
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

// ---------------------------------------------------------- kinematic bicycle --
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

}  // namespace mpcqp
