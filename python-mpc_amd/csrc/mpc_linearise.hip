// mpc_linearise.hip -- the MPC data path around the solver, on the device:
// the linearisations of the two vehicle models (vehicle_model.h), batched over B vehicles, with
// their transposes in the point and in the vehicle's constants, and the fleet objects.
//
//   F2  k_linearise<DynamicBicycle>   Vehicle_Dynamics.get_dynamics_model  vehicle_models.py:52-340
//       k_linearise<KinematicBicycle> Vehicle_Kinematics.get_kinematics_model vehicle_models.py:835-863
// and the gradients with respect to the vehicle's constants, in fleet form:
//       k_linearise_pvjp / k_kin_linearise_pvjp   the linearisations, summed over the stages
//       k_euler_step_pvjp / k_kin_update_pvjp     the terminal steps of the three loop tails
// The two bicycles are model structs (DynamicBicycle, KinematicBicycle) over which the
// linearisation is written once.
//
// One thread per (vehicle, stage) for the linearisation.  All fp64.
//
// Each host template below is followed by the entry points that forward to it, the uniform one and
// its _fleet twin.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <type_traits>
#include <vector>

#include "../../include/mpcqp.h"
#include "kernels.h"
#include "mpc_fleet.h"
#include "mpc_host.h"
#include "vehicle_model.h"

namespace mpcqp {

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

// VJP of linearise_one(const mpcqp_kin_vehicle&, ...) per (vehicle, stage): only v, yaw and steer
// carry derivative; the outputs are dense (B, N, 4) / (B, N, 2) whatever the input strides.
// A template over the constants' source KS (the struct, or a fleet's TableK), as every kernel of
// the data path that takes a vehicle and is not a template over its model or Tail already.
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

}  // namespace mpcqp

using namespace mpcqp;

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
}  // extern "C"

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

extern "C" {
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
}  // extern "C"

// ---- gradients with respect to a fleet's constants: fleet form only ----

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

extern "C" {
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
}  // extern "C"

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

extern "C" {
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

// ---- fleets: one table of constants per batch (mpc_fleet.h) ----

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

extern "C" {
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
}  // extern "C"

template <class F>
void fleet_free(F* f) {
    if (!f) return;
    if (f->d_k) {
        (void)hipSetDevice(f->dev);
        (void)hipFree(f->d_k);
    }
    delete f;
}

extern "C" {
void mpcqp_fleet_free(mpcqp_fleet* f) { fleet_free(f); }
void mpcqp_kin_fleet_free(mpcqp_kin_fleet* f) { fleet_free(f); }
}  // extern "C"
