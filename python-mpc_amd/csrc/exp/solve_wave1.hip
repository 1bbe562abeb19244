// solve_wave1.hip -- the ADMM kernel with ONE 64-lane wavefront per QP instance.
//
// Why a wave and not a workgroup: one ADMM iteration of a cfg-2 QP (SURVEY.md §8,
// n = 104, m = 188) is ~7 kFLOP of dependent phases (rhs gather, block solve, row
// update).  Spread over a 256-thread workgroup (solve.hip) every phase boundary
// is an s_barrier between four waves and the iteration costs ~7,000 cycles, almost
// all of it barrier and LDS round trips.  Inside a single wave the phases are
// ordered by the wave's own instruction stream: the compiler drops s_barrier for a
// 64-thread workgroup (it emits only the LDS waitcnt), so a phase boundary costs one
// LDS round trip, and each wave is an independent QP that the four SIMDs of a CU
// run side by side.
//
// Work decomposition (NB <= 4 blocks of S = 32 variables, amax <= 8 coupling rows):
//   lane = (h, r) = (lane / 32, lane % 32) owns the padded columns
//     pc_e = kb_e * 32 + r,  kb_0 = h, kb_1 = 3 - h   (blocks {0,3} / {1,2}: balanced
//     phase-C work), with x, x_prev, q and its column gather lists in registers;
//   constraint rows i = lane + 64 s (s < RS) with y, z, their row gather lists;
//   the factor, in the three-phase form K^{-1} = L^{-T} D^{-1} L^{-1}
//   (solve_phases.h::factorize, mode 2):
//     SB[e][c] = S_{kb_e}^{-1}[r][c]                        (phase B, 64 doubles)
//     GA[q][e] = G_q[lane / 8][4 (lane % 8) + e]            (phase A, pair q = k(k-1)/2 + j)
//     GC[s][q] = G_{j_s, kb_s}[q][r]                        (phase C, transposed use)
// One iteration:
//   rhs   b = sigma x - q + A'(rho z - y)                   -> rb   (LDS)
//   A     c_k = sum_{j<k} G_kj b_j   (8-lane DPP sums)      -> cor  (LDS)
//   B     t_k = S_k^{-1} (b_k + c_k)                        -> tv   (LDS)
//   C     x~_k = t_k + sum_{j>k} G_jk' t_j                  -> xt   (LDS)
//   rows  z~ = A x~, relaxation, projection, y update, w = rho z - y -> w (LDS)
// Reference semantics as solve.hip (OSQP 0.6 osqp_solve, behind
// vehicle_lateral_mpc_slack_increment.py:248 / Control/MPC/mpc_dynamics.py:396).
// Variants 8 and 9: measured and not taken, the experimental builds only.
#include <hip/hip_runtime.h>

#include "../solve_phases.h"
#include "../wave_util.h"
#include "exp.h"

namespace mpcqp {

constexpr int TW = 64;

// S^{-1} rows of the lane's two blocks, SB[e][c] = S_{kb_e}^{-1}[r][c] (128 VGPRs)
struct WaveFactor {
    double SB[2][S];
    __device__ __forceinline__ void load(const double* __restrict__ Sg) {
        const int lane = threadIdx.x, h = lane >> 5, r = lane & 31;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double* src = Sg + (long)(e ? 3 - h : h) * SS + r * S;
#pragma unroll
            for (int c = 0; c < S; ++c) SB[e][c] = src[c];
        }
    }
};

template <int K, int RS>
__global__ __launch_bounds__(TW, 1) void k_solve_w(KParams p, double* __restrict__ xo, double* __restrict__ yo,
                                                   int factor_only) {
    const int lane = threadIdx.x;
    const int h = lane >> 5, r = lane & 31, rr = lane >> 3, ch = lane & 7;
    const int kb0 = h, kb1 = 3 - h;
    constexpr int NB = 4, NP = NB * (NB - 1) / 2;  // exactly four blocks (solve.hip::variant_fits)
    const long b = instance_of(p);
    const int m = p.m, npad = p.npad, nnzA = p.nnzA;
    SL2 C = carve(p);
    SLds& L = C.L;
    const double* Hg = p.H + b * (long)p.nb * SS;
    const double* Sg = p.Si + b * (long)p.nb * SS;

    if (p.err[b]) {  // invalid data (flagged by setup/update): NaN outputs
        reject_instance<TW>(p, b, xo, yo);
        return;
    }

    PROF_START

    const double cval = p.scal[b * 4 + 0], cinv = p.scal[b * 4 + 1];
    double rho = p.scal[b * 4 + 2];
    const double sigma = p.sigma, alpha = p.alpha;
    const bool warm = p.warm_start != 0;
    const int mp = solve_mpad(m);
    load_instance<TW>(p, b, C, warm);
    if (lane < S) L.cor[lane] = 0.0;  // block 0 has no phase-A correction

    int status = MPCQP_UNSOLVED_, rho_updates = 0, iter = 0, info_iter = 0;
    bool can_check = false, need_factor = true;
    PH(5)
    // Runs of ADMM iterations up to the next termination / rho-adaptation point
    // alternate with the out-of-line phases; the run state lives in registers and
    // is re-derived from LDS and the workspace at every run start (nothing but
    // scalars is live across a call).
    for (;;) {
        __syncthreads();
        if (need_factor) {  // start, and after a rho change
            need_factor = false;
            // the factorisation scratch aliases ys (and dY, rb, xt, w): y waits in the
            // workspace's y array (the warm-start input at the first factorisation)
            if (iter > 0)
                for (int i = lane; i < m; i += TW) p.y[b * m + i] = L.ys[i];
            const bool ok = factorize_nl<TW>(p.self, b, rho);
            if (!ok) {
                if (iter == 0) {
                    reject_instance<TW>(p, b, xo, yo);
                    return;
                }
                status = MPCQP_NON_CVX_;
                can_check = true;  // skip the final check_termination
                break;
            }
            if (factor_only) return;
            __syncthreads();
            const bool have_y = iter > 0 || warm;
            for (int i = lane; i < mp; i += TW) L.ys[i] = (have_y && i < m) ? p.y[b * m + i] : 0.0;
            // G blocks -> LDS, rows padded to 8 with zeros: gl[pair][row < 8][32]
            for (int o = lane; o < NP * 8 * S; o += TW) {
                const int q = o >> 8, t = (o >> 5) & 7;
                L.gl[o] = t < p.amax ? Hg[(long)q * p.amax * S + (o & 255)] : 0.0;
            }
            PH(0)
        }
        // ---- run state ----
        WaveFactor RF;
        RF.load(Sg);
        int pcs[2];
        bool cv[2];
        double X[2], Q[2], DX[2];
        // LDS byte addresses of the gathered arrays
        const unsigned abase = lds_addr(L.Acsc), wbase = lds_addr(L.w), xbase = lds_addr(L.xt);
        GatherW<K> cg[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int pc = (e ? kb1 : kb0) * S + r;  // < npad = 4 S
            pcs[e] = pc;
            cv[e] = p.pad_var[pc] >= 0;
            X[e] = C.X[pc];
            Q[e] = L.qv[pc];
            DX[e] = 0.0;
            cg[e].load(p.gcol + pc, npad, abase, wbase);
        }
        GatherW<K> rg[RS];
        double y[RS], Z[RS], dy[RS], rv[RS], rvi[RS];
        const double r_hi = RHO_EQ_OVER_RHO_INEQ * rho;
#pragma unroll
        for (int s = 0; s < RS; ++s) {
            const int i = lane + s * TW;  // < mp
            dy[s] = 0.0;
            if (i < m) rg[s].load(p.grow + i, m, abase, xbase);
            else rg[s].clear(abase + 8u * nnzA, xbase);
            y[s] = L.ys[i];
            Z[s] = C.Z[i];
            const signed char cl = L.ct[i];  // OSQP rho_vec / rho_inv_vec of the row
            rv[s] = cl < 0 ? RHO_MIN : (cl > 0 ? r_hi : rho);
            rvi[s] = cl < 0 ? 1.0 / RHO_MIN : (cl > 0 ? 1.0 / r_hi : 1.0 / rho);
            L.w[i] = rv[s] * Z[s] - y[s];  // w = rho z_prev - y (rho may be new)
        }
        const int stop_at = run_stop(p, iter);
        __syncthreads();
        PH(5)
        while (iter < stop_at) {
            ++iter;
            int opq = 0;
            asm volatile("" : "+s"(opq));  // keeps per-lane LDS addresses out of the register budget
            double* const rb = L.rb + opq;
            double* const cor = L.cor + opq;
            double* const tv = L.tv + opq;
            double* const xt = L.xt + opq;
            // rhs = sigma x_prev - q + A' (rho z_prev - y)
            {
                double av[2][K], wv[2][K];
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        av[e][k] = lds_at(cg[e].e[k] & 0xFFFFu);
                        wv[e][k] = lds_at(cg[e].e[k] >> 16);
                    }
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    double v = sigma * X[e] - Q[e];
#pragma unroll
                    for (int k = 0; k < K; ++k) v += av[e][k] * wv[e][k];
                    rb[pcs[e]] = cv[e] ? v : 0.0;
                }
            }
            __syncthreads();
            PH(1)
            // A: c_k = sum_{j<k} G_kj b_j on rows < 8: lane (rr, ch) takes columns
            // [4 ch, 4 ch + 4) of every pair, 8-lane DPP sums over ch (every lane of
            // the group holds the sum and writes it)
            {
                const double* gq = L.gl + opq + rr * S + 4 * ch;
                double bj[NB - 1][4], ga[NP][4];
#pragma unroll
                for (int j = 0; j < NB - 1; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) bj[j][e] = rb[j * S + 4 * ch + e];
#pragma unroll
                for (int q = 0; q < NP; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) ga[q][e] = gq[q * 8 * S + e];
#pragma unroll
                for (int k = 1; k < NB; ++k) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < k; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc += ga[k * (k - 1) / 2 + j][e] * bj[j][e];
                    cor[k * S + rr] = reduce8(acc);
                }
            }
            __syncthreads();
            // B: t_kb = S_kb^{-1} (b_kb + c_kb), one full row per lane and block
            double t[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int kb = e ? kb1 : kb0;
                const double* bv = rb + kb * S;
                const double* cb = cor + kb * S;
                double v[S], cc[8];
#pragma unroll
                for (int c = 0; c < S; ++c) v[c] = bv[c];
#pragma unroll
                for (int c = 0; c < 8; ++c) cc[c] = cb[c];
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] += cc[c];
                double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < S; ++c) a[c & 3] += RF.SB[e][c] * v[c];
                t[e] = (a[0] + a[1]) + (a[2] + a[3]);
            }
            tv[kb0 * S + r] = t[0];
            tv[kb1 * S + r] = t[1];
            __syncthreads();
            // C: x~_kb = t_kb + sum_{j>kb} G_{j,kb}' t_j  (t_j rows < 8); the lane's
            // pairs: h = 0: (1,0) (2,0) (3,0);  h = 1: (2,1) (3,1) (3,2)
            double xn[2];
            {
                double d[3], gv[3][8], tq[3][8];
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    const int j = s < 2 ? s + 1 + h : 3;
                    const int kb = s < 2 ? h : 2 * h;
                    const double* tj = tv + j * S;
                    const double* gc = L.gl + opq + (j * (j - 1) / 2 + kb) * 8 * S + r;
#pragma unroll
                    for (int q = 0; q < 8; ++q) { gv[s][q] = gc[q * S]; tq[s][q] = tj[q]; }
                }
#pragma unroll
                for (int s = 0; s < 3; ++s) {
                    double a0 = 0.0, a1 = 0.0;
#pragma unroll
                    for (int q = 0; q < 8; q += 2) {
                        a0 += gv[s][q] * tq[s][q];
                        a1 += gv[s][q + 1] * tq[s][q + 1];
                    }
                    d[s] = a0 + a1;
                }
                xn[0] = t[0] + (d[0] + d[1]) + (h ? 0.0 : d[2]);
                xn[1] = t[1] + (h ? d[2] : 0.0);
            }
            xt[kb0 * S + r] = xn[0];
            xt[kb1 * S + r] = xn[1];
            // x update (own columns, registers)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const double xnew = alpha * xn[e] + (1.0 - alpha) * X[e];
                DX[e] = xnew - X[e];
                X[e] = xnew;
            }
            __syncthreads();
            PH(2)
            // z~ = A x~ ; relaxed + projected z ; y ; next w   (padded rows stay 0)
            double zts[RS];
            {
                double av[RS][K], xv[RS][K];
#pragma unroll
                for (int s = 0; s < RS; ++s)
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        av[s][k] = lds_at(rg[s].e[k] & 0xFFFFu);
                        xv[s][k] = lds_at(rg[s].e[k] >> 16);
                    }
#pragma unroll
                for (int s = 0; s < RS; ++s) {
                    double v = av[s][0] * xv[s][0];
#pragma unroll
                    for (int k = 1; k < K; ++k) v += av[s][k] * xv[s][k];
                    zts[s] = v;
                }
            }
#pragma unroll
            for (int s = 0; s < RS; ++s) {
                const int i = lane + opq + s * TW;
                const double zt = zts[s];
                const double zr = alpha * zt + (1.0 - alpha) * Z[s];
                const double zn = __builtin_fmin(__builtin_fmax(zr + rvi[s] * y[s], L.lo[i]), L.up[i]);
                const double dd = rv[s] * (zr - zn);
                Z[s] = zn;
                dy[s] = dd;
                y[s] += dd;
                L.w[i] = rv[s] * zn - y[s];
            }
            __syncthreads();
            PH(3)
        }
        // run state back to LDS for the out-of-line phases
#pragma unroll
        for (int e = 0; e < 2; ++e) { C.X[pcs[e]] = X[e]; L.dx[pcs[e]] = DX[e]; }
#pragma unroll
        for (int s = 0; s < RS; ++s) {
            const int i = lane + s * TW;
            L.ys[i] = y[s]; C.Z[i] = Z[s]; C.dY[i] = dy[s];
        }
        __syncthreads();
        // ---- out-of-line phases (only scalars live across these calls) ----
        can_check = p.check_term && (iter % p.check_term == 0);
        const bool do_rho = p.adaptive_rho && p.rho_interval && (iter % p.rho_interval == 0);
        if (!can_check && !do_rho) break;  // max_iter reached
        info_iter = iter;
        const bool stop = check_and_adapt<TW>(p, b, L, cval, cinv, can_check, do_rho, status, rho, rho_updates,
                                                need_factor);
        __syncthreads();
        PH(4)
        if (stop || iter >= p.max_iter) break;
    }
    conclude<TW>(p, b, xo, yo, cval, cinv, rho, status, can_check, iter, info_iter, rho_updates);
#ifdef MPCQP_PHASE_PROF
    if (prof) {
        __syncthreads();
        PH(5)
        if (lane == 0) {
            prof_flush(p, b, L, t0c, t0w, 11);
        }
    }
#endif
}

template <int K, int RS>
static hipError_t go_w(const KParams& p, long B, double* xo, double* yo, int fo, hipStream_t st, size_t lds,
                       KernelRef* ref) {
    auto k = k_solve_w<K, RS>;
    if (ref) { *ref = {(const void*)k, TW, lds}; return hipSuccess; }
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(TW), lds, st, p, xo, yo, fo);
    return hipGetLastError();
}

hipError_t launch_solve_wave1(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                              KernelRef* ref) {
    const size_t lds = lds_solve_bytes(p);
    switch (p.variant) {
        case 8: return go_w<6, 3>(p, B, xo, yo, factor_only, st, lds, ref);
        case 9: return go_w<8, 4>(p, B, xo, yo, factor_only, st, lds, ref);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace mpcqp
