// adjoint.hip -- gradients of the batched QP solution (mpcqp_adjoint_device).
//
// At a solved instance with active rows A_act (the row classes below), the solution map
// (P, q, A, l, u) -> (x, y) is locally the linear system  K [x; y_act] = [-q; b_act],
// K = [[P, A_act'], [A_act, 0]]  (b_act the active bounds), so the gradient of
// L = g_x . x + g_y . y  with respect to the data is one solve with K (symmetric) per seed:
//     K [r_x; r_y] = [g_x; g_y],   r_y = 0 on inactive rows,
//     dL/dq = -r_x,   dL/dl_i or dL/du_i = r_y,i (the active side),
//     dL/dA_ij = -(y_i r_x,j + r_y,i x_j),   dL/dP_ij = -(r_x,i x_j + r_x,j x_i)  (i < j),
//     dL/dP_ii = -r_x,i x_i.
// The solve is polish's (solve.hip::k_polish): the delta-regularised reduced matrix
//     P + delta I + A_act' A_act / delta
// factored once per instance by factorize<POL> into the workspace tiles, then per seed the
// eliminated solve and polish_refine_iter refinement steps against the unregularised K.
// Everything runs on the scaled data of the workspace (P~ = c D P D, A~ = E A D, x = D x~,
// y = E y~ / c) with the seeds (D g_x, E g_y / c); r_x = c D r~_x and r_y = E r~_y then
// satisfy the unscaled equations above, and the gradients are formed from unscaled values.
//
// Row classes (scaled data, the workspace's z and y, as polish's form_Ared):
//   3 equality  l == u, always active, counted once (polish counts it twice);
//   1 lower     z - l < -y;      2 upper     u - z < y;      0 inactive.
//
// One 256-thread workgroup per instance, polish's LDS carve.  Like polish the kernel takes the
// workspace factor tiles (ffresh = 0) and touches no iterate, info or status.
#include <hip/hip_runtime.h>

#include "solve_phases.h"

namespace mpcqp {

namespace {

constexpr double kAdjTol = 1e-8;    // astat = 1: every seed's relative residual below this
constexpr double kAdjTiny = 1e-300; // floor of the seed norm (a zero seed: residual 0)

// zeros in every output of instance b's seed r (an instance that is not solved, a failed
// factorisation, a solve that did not stay finite)
__device__ __forceinline__ void adjoint_zero(const KParams& p, const AdjointIO& io, long b, int r) {
    const int tid = threadIdx.x, n = p.n, m = p.m;
    const long s = b * io.nrhs + r;
    for (int j = tid; j < n; j += T) {
        if (io.rx) io.rx[s * n + j] = 0.0;
        if (io.gq) io.gq[s * n + j] = 0.0;
    }
    for (int i = tid; i < m; i += T) {
        if (io.ry) io.ry[s * m + i] = 0.0;
        if (io.gl) io.gl[s * m + i] = 0.0;
        if (io.gu) io.gu[s * m + i] = 0.0;
    }
    if (io.gPx) for (int v = tid; v < p.nnzP; v += T) io.gPx[s * p.nnzP + v] = 0.0;
    if (io.gAx) for (int v = tid; v < p.nnzA; v += T) io.gAx[s * p.nnzA + v] = 0.0;
}

}  // namespace

__global__ __launch_bounds__(T) void k_adjoint(KParams p, AdjointIO io) {
    const int tid = threadIdx.x;
    const long b = blockIdx.x;
    const int n = p.n, m = p.m, npad = p.npad, nnzP = p.nnzP, nnzA = p.nnzA, nrhs = io.nrhs;
    if (p.status[b] != MPCQP_SOLVED_) {
        for (int r = 0; r < nrhs; ++r) {
            adjoint_zero(p, io, b, r);
            if (tid == 0 && io.ares) io.ares[b * nrhs + r] = 0.0;
        }
        if (io.act) for (int i = tid; i < m; i += T) io.act[b * m + i] = 0;
        if (tid == 0 && io.astat) io.astat[b] = 0;
        return;
    }
    SL2 C = carve(p);
    SLds& L = C.L;
    double* SX = C.X;     // r~_x
    double* SY = C.Z;     // r~_y (zero on inactive rows)
    double* AX = C.dY;    // A~ r~_x of the refinement step
    double* GX = L.qv;    // scaled seed D g_x
    double* GY = L.up;    // scaled seed E g_y / c on active rows, zero elsewhere
    double* CLS = L.lo;   // row class + 4 (l infinite) + 8 (u infinite), kept across the factorisation
    double* XU = L.tv;    // unscaled x by padded column
    const double cval = p.scal[b * 4 + 0], cinv = p.scal[b * 4 + 1], idelta = 1.0 / p.delta;
    const double* Fg = p.F + b * (long)p.nb * SS;
    const double* Sg = p.Si + b * (long)p.nb * SS;
    const double* Eg = p.E + b * m;
    const double* Dg = p.D + b * npad;
    const bool sc = p.scaling != 0;
    for (int e = tid; e < nnzA; e += T) L.Acsc[e] = p.Ax[b * nnzA + e];
    if (tid == 0) L.Acsc[nnzA] = 0.0;
    for (int v = tid; v < nnzP; v += T) L.Pv[v] = p.Px[b * nnzP + v];
    if (tid == 0) L.Pv[nnzP] = 0.0;
    const double inf_s = OSQP_INFTY * MIN_SCALING;  // OSQP's bound-is-infinite test on scaled data
    for (int i = tid; i < m; i += T) {
        const double lo = p.l[b * m + i], up = p.u[b * m + i], z = p.z[b * m + i], y = p.y[b * m + i];
        const int cls = lo == up ? 3 : (z - lo < -y ? 1 : (up - z < y ? 2 : 0));
        CLS[i] = (double)(cls | (lo <= -inf_s ? 4 : 0) | (up >= inf_s ? 8 : 0));
        // factorize<POL>'s row weight is the number of set bits 0 / 1: one for every active row
        L.ct[i] = (signed char)(cls == 3 ? 1 : cls);
        if (io.act) io.act[b * m + i] = (signed char)cls;
    }
    if (tid == 0) p.ffresh[b] = 0;  // the adjoint system's factor takes the workspace tiles
    __syncthreads();
    const bool ok = factorize_pol_nl<T>(p.self, b);
    if (!ok) {  // not quasi-definite: nothing is solved (zeros have relative residual 1)
        for (int r = 0; r < nrhs; ++r) {
            adjoint_zero(p, io, b, r);
            if (tid == 0 && io.ares) io.ares[b * nrhs + r] = 1.0;
        }
        if (tid == 0 && io.astat) io.astat[b] = -1;
        return;
    }
    for (int pc = tid; pc < npad; pc += T) XU[pc] = sc ? Dg[pc] * p.x[b * npad + pc] : p.x[b * npad + pc];
    bool all_ok = true;
    for (int r = 0; r < nrhs; ++r) {
        const long s = b * nrhs + r;
        __syncthreads();  // the previous seed's output phase read w, rb, ys
        double nrm[2] = {0.0, 0.0};  // [0] the seed's norm, [1] the residual's
        for (int pc = tid; pc < npad; pc += T) {
            const int j = p.pad_var[pc];
            const double g = (j >= 0 && io.gx) ? (sc ? Dg[pc] * io.gx[s * n + j] : io.gx[s * n + j]) : 0.0;
            GX[pc] = g;
            SX[pc] = 0.0;
            nrm[0] = cmax(nrm[0], fabs(g));
        }
        for (int i = tid; i < m; i += T) {
            const bool act = ((int)CLS[i] & 3) != 0;
            const double g = (act && io.gy) ? (sc ? (Eg[i] * io.gy[s * m + i]) * cinv : io.gy[s * m + i]) : 0.0;
            GY[i] = g;
            SY[i] = 0.0;
            nrm[0] = cmax(nrm[0], fabs(g));
        }
        __syncthreads();
        for (int it = 0; it <= p.refine_iter; ++it) {
            // residual of K s = g folded into the eliminated rhs: r_x + A_act' r_y / delta
            for (int i = tid; i < m; i += T) {
                const bool act = ((int)CLS[i] & 3) != 0;
                const double ax = row_dot(p, L.Acsc, SX, i);
                AX[i] = ax;
                L.w[i] = act ? (GY[i] - ax) * idelta - SY[i] : 0.0;
            }
            __syncthreads();
            for (int pc = tid; pc < npad; pc += T)
                L.rb[pc] = p.pad_var[pc] >= 0 ? (GX[pc] - psym_dot(p, L.Pv, SX, pc)) + col_dot(p, L.Acsc, L.w, pc)
                                              : 0.0;
            __syncthreads();
            pol_solve(p, Fg, Sg, L.rb, L.xt);
            for (int i = tid; i < m; i += T) {  // dy = (A_act dx - r_y) / delta
                if (((int)CLS[i] & 3) == 0) continue;
                SY[i] += (row_dot(p, L.Acsc, L.xt, i) - (GY[i] - AX[i])) * idelta;
            }
            __syncthreads();
            for (int pc = tid; pc < npad; pc += T) SX[pc] += L.xt[pc];
            __syncthreads();
        }
        // || K s - g ||_inf on the scaled system
        // (a NaN or an infinity is flagged on its own: the maxima's comparisons drop a NaN)
        bool bad = false;
        for (int i = tid; i < m; i += T) {
            if (((int)CLS[i] & 3) == 0) continue;
            const double v = fabs(row_dot(p, L.Acsc, SX, i) - GY[i]);
            bad = bad || !(v < OSQP_INFTY) || !(fabs(SY[i]) < OSQP_INFTY);
            nrm[1] = cmax(nrm[1], v);
        }
        for (int pc = tid; pc < npad; pc += T) {
            if (p.pad_var[pc] < 0) continue;
            const double v = fabs((psym_dot(p, L.Pv, SX, pc) + col_dot(p, L.Acsc, SY, pc)) - GX[pc]);
            bad = bad || !(v < OSQP_INFTY) || !(fabs(SX[pc]) < OSQP_INFTY);
            nrm[1] = cmax(nrm[1], v);
        }
        block_max<T>(nrm, L.red);
        bad = block_any<T>(bad, L.flag);
        const double ares = bad ? 1.0 : nrm[1] / cmax(nrm[0], kAdjTiny);
        all_ok = all_ok && ares < kAdjTol;
        if (tid == 0 && io.ares) io.ares[s] = ares;
        if (bad) {  // the solve did not stay finite: zeros (relative residual 1)
            adjoint_zero(p, io, b, r);
            continue;
        }
        // unscaled r_x by padded column (rb), r_y (w) and y (ys)
        for (int pc = tid; pc < npad; pc += T) L.rb[pc] = sc ? cval * (Dg[pc] * SX[pc]) : SX[pc];
        for (int i = tid; i < m; i += T) {
            L.w[i] = sc ? Eg[i] * SY[i] : SY[i];
            L.ys[i] = sc ? (Eg[i] * p.y[b * m + i]) * cinv : p.y[b * m + i];
        }
        __syncthreads();
        for (int pc = tid; pc < npad; pc += T) {
            const int j = p.pad_var[pc];
            if (j < 0) continue;
            if (io.rx) io.rx[s * n + j] = L.rb[pc];
            if (io.gq) io.gq[s * n + j] = -L.rb[pc];
        }
        for (int i = tid; i < m; i += T) {
            const int code = (int)CLS[i], cls = code & 3;
            const double ry = L.w[i];
            // an equality row's r_y goes to the side its dual points at
            const bool to_l = cls == 1 || (cls == 3 && !(L.ys[i] > 0.0));
            const bool to_u = cls == 2 || (cls == 3 && L.ys[i] > 0.0);
            if (io.ry) io.ry[s * m + i] = ry;
            if (io.gl) io.gl[s * m + i] = (to_l && !(code & 4)) ? ry : 0.0;
            if (io.gu) io.gu[s * m + i] = (to_u && !(code & 8)) ? ry : 0.0;
        }
        if (io.gAx)
            for (int v = tid; v < nnzA; v += T) {
                const int i = p.a_r[v], pc = p.a_c[v];
                io.gAx[s * nnzA + v] = -(L.ys[i] * L.rb[pc] + L.w[i] * XU[pc]);
            }
        if (io.gPx)
            for (int v = tid; v < nnzP; v += T) {
                const int pr = p.p_r[v], pc = p.p_c[v];
                io.gPx[s * nnzP + v] = pr == pc ? -(L.rb[pr] * XU[pr]) : -(L.rb[pr] * XU[pc] + L.rb[pc] * XU[pr]);
            }
    }
    if (tid == 0 && io.astat) io.astat[b] = all_ok ? 1 : -1;
}

hipError_t launch_adjoint(const KParams& p, long B, const AdjointIO& io, hipStream_t st) {
    const size_t lds = lds_solve_bytes(p);
    hipError_t e = hipFuncSetAttribute((const void*)k_adjoint, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_adjoint, dim3((unsigned)B), dim3(T), lds, st, p, io);
    return hipGetLastError();
}

}  // namespace mpcqp
