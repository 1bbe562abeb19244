// solve_wave.hip -- the ADMM kernels with one wavefront per block of the QP: the two-wave
// kernel (variant 10: a 128-thread workgroup per QP, each wave two blocks) and the four-wave
// kernel (variant 17: a 256-thread workgroup, one block per wave), each with its fused
// setup + solve form.  The one-wave and eight-wave kernels they grew out of and after were
// measured and not taken: exp/solve_wave1.hip, exp/solve_wave8.hip (the experimental builds).
// Reference semantics as solve.hip (OSQP 0.6 osqp_solve, behind
// vehicle_lateral_mpc_slack_increment.py:248 / Control/MPC/mpc_dynamics.py:396).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "setup_r.h"
#include "solve_phases.h"
#include "wave_util.h"

namespace mpcqp {

// ---------------------------------------------------------------------------
// Two-wave variant: one 128-thread workgroup (2 waves, on 2 SIMDs) per QP.
// Wave w owns blocks {0, 3} (w = 0) or {1, 2} (w = 1), one block row per lane
// (lane = (h, r): block kb = w ? 1 + h : 3 h, row r), so each wave issues half the
// work of the one-wave kernel with half its registers.  The waves meet at three
// workgroup barriers per iteration (after rhs, after x~, after the row update);
// the cross-block terms of the solve that a wave needs from the other wave's
// blocks (c_k of phase A, and the rows < 8 of t_j that phase C reads) are
// recomputed inside the wave instead of exchanged: phase A is done by both
// waves, and wave 0 recomputes t_1, t_2 (rows < 8), wave 1 recomputes t_3.
// Per-wave LDS for those: cw[w][block][8] (in cor), tw[w][block][8] (in tv).
constexpr int T2 = 128;

template <int K, int RS, int KPK, int K1>
__device__ __forceinline__ void solve_w2_body(const KParams& p, double* __restrict__ xo, double* __restrict__ yo,
                                              int factor_only) {
    static_assert(RS == 2, "rows i = tid and tid + 128");
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const int h = lane >> 5, r = lane & 31, rr = lane >> 3, ch = lane & 7;
    const int kb = w ? 1 + h : 3 * h;          // own block
    const int jr = w ? 3 : 1 + h;              // block of the recomputed t rows
    const int rq = r >> 2, cq = r & 3;         // recomputed row / column chunk
    constexpr int NB = 4, NP = NB * (NB - 1) / 2;  // exactly four blocks (solve.hip::variant_fits)
    const long b = instance_of(p);
    const int m = p.m, npad = p.npad, nnzA = p.nnzA;
    SL2 C = carve(p);
    SLds& L = C.L;
    const double* Hg = p.H + b * (long)p.nb * SS;
    // S_k^{-1} stays in LDS after the carve (lds_w2_bytes): at one wave per SIMD two
    // workgroups share a CU, so the LDS is there; nothing goes to / comes from the workspace
    double* const Sg = w4_tiles(p, C);

    if (p.err[b]) {  // invalid data (flagged by setup/update): NaN outputs
        reject_instance<T2>(p, b, xo, yo);
        return;
    }
    PROF_START

    const double cval = p.scal[b * 4 + 0], cinv = p.scal[b * 4 + 1];
    double rho = p.scal[b * 4 + 2];
    const double sigma = p.sigma, alpha = p.alpha;
    const bool warm = p.warm_start != 0;
    const int mp = solve_mpad(m);
    load_instance<T2>(p, b, C, warm);
    if (tid < 16) L.cor[(tid >> 3) * 32 + (tid & 7)] = 0.0;  // cw[w][0][*]: block 0 has no correction

    int status = MPCQP_UNSOLVED_, rho_updates = 0, iter = 0, info_iter = 0;
    bool can_check = false, need_factor = true;
    // Loop-invariant per-lane data from global memory (the plan's gather lists, the
    // scalings D and E): loaded after each factorisation (which is a call: nothing
    // vector-valued is live across it), kept in registers across the runs and the
    // inline termination checks in between.
    const int pc = kb * S + r;
    const unsigned abase = lds_addr(L.Acsc), wbase = lds_addr(L.w), xbase = lds_addr(L.xt);
    const unsigned Xbase = lds_addr(C.X);
    bool cv = false;
    double Dv = 1.0, Ev[RS];
    // row gather lists: slot 0 (rows < 128) K entries, slot 1 (rows >= 128) K1 <= K --
    // the plan's row order often puts the short rows last (cfg 2: the box rows, one
    // nonzero each, are rows 84..187), so slot 1 skips the zero-padded entries
    GatherW<K> cg, rg0;
    GatherW<K1> rg1;
    GatherW<KPK> pg;  // the column's P list (addresses of Pv / X), for the inline check
    PH(5)
    for (;;) {
        __syncthreads();
        if (need_factor) {  // start, and after a rho change
            need_factor = false;
            // the factorisation scratch aliases ys: y waits in the workspace's y array
            if (iter > 0) {
                for (int i = tid; i < m; i += T2) p.y[b * m + i] = L.ys[i];
                __syncthreads();  // every ys read is done before factorize_w2's scratch overwrites it
            }
            const bool ok = factorize_nl<T2>(p.self, b, rho, Sg);
            if (!ok) {
                if (iter == 0) {
                    reject_instance<T2>(p, b, xo, yo);
                    return;
                }
                status = MPCQP_NON_CVX_;
                can_check = true;  // skip the final check_termination
                break;
            }
            if (factor_only) return;
            __syncthreads();
            const bool have_y = iter > 0 || warm;
            for (int i = tid; i < mp; i += T2) L.ys[i] = (have_y && i < m) ? p.y[b * m + i] : 0.0;
            // G blocks -> LDS, rows padded to 8 with zeros, plus one all-zero pair (index NP):
            // gl[pair][row < 8][32]
            for (int o = tid; o < (NP + 1) * 8 * S; o += T2) {
                const int q = o >> 8, t = (o >> 5) & 7;
                L.gl[o] = (q < NP && t < p.amax) ? Hg[(long)q * p.amax * S + (o & 255)] : 0.0;
            }
            cv = p.pad_var[pc] >= 0;
            cg.load(p.gcol + pc, npad, abase, wbase);
            pg.load(p.gpsym + pc, npad, lds_addr(L.Pv), Xbase);
            Dv = p.D[b * npad + pc];
#pragma unroll
            for (int s = 0; s < RS; ++s) {
                const int i = min(tid + s * T2, mp - 1);
                Ev[s] = i < m ? p.E[b * m + i] : 1.0;
            }
            {
                const int i0 = tid, i1 = min(tid + T2, mp - 1);
                if (i0 < m) rg0.load(p.grow + i0, m, abase, xbase);
                else rg0.clear(abase + 8u * nnzA, xbase);
                if (i1 < m) rg1.load(p.grow + i1, m, abase, xbase);
                else rg1.clear(abase + 8u * nnzA, xbase);
            }
            PH(0)
        }
        // ---- run state ----
        double SB[S], SR[8];
        {
            const double* src = Sg + (long)kb * SS + r * S;
#pragma unroll
            for (int c = 0; c < S; c += 2) ld2(src + c, SB[c], SB[c + 1]);
            const double* srr = Sg + (long)jr * SS + rq * S + 8 * cq;
#pragma unroll
            for (int i = 0; i < 8; i += 2) ld2(srr + i, SR[i], SR[i + 1]);
        }
        double X = C.X[pc], DX = 0.0;
        const double Q = L.qv[pc];
        // phase-C slots (pair, j) of the lane; pair NP is the zero block.  Block 0 needs
        // three pairs and block 3 none, so wave 0's upper half (block 3's rows) takes block
        // 0's pair (3,0) and hands its partial sum over with a half-wave swap: two slots
        // per lane in both waves.
        int gslot[2], tslot[2];
        {
            int pr[2], jj[2];
            if (w == 0 && h == 0) { pr[0] = 0; jj[0] = 1; pr[1] = 1; jj[1] = 2; }
            else if (w == 0)      { pr[0] = 3; jj[0] = 3; pr[1] = NP; jj[1] = 3; }
            else if (h == 0)      { pr[0] = 2; jj[0] = 2; pr[1] = 4; jj[1] = 3; }
            else                  { pr[0] = 5; jj[0] = 3; pr[1] = NP; jj[1] = 3; }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                gslot[s] = lds_addr(L.gl + pr[s] * 8 * S + r);
                tslot[s] = lds_addr(L.tv + w * 32 + jj[s] * 8);
            }
        }
        double y[RS], Z[RS], dy[RS], rv[RS], rvi[RS];
        int ri[RS];
        const double r_hi = RHO_EQ_OVER_RHO_INEQ * rho;
#pragma unroll
        for (int s = 0; s < RS; ++s) {
            const int i = min(tid + s * T2, mp - 1);  // lanes past the padded rows repeat the inert last row
            ri[s] = i;
            dy[s] = 0.0;
            y[s] = L.ys[i];
            Z[s] = C.Z[i];
            const signed char cl = L.ct[i];  // OSQP rho_vec / rho_inv_vec of the row
            rv[s] = cl < 0 ? RHO_MIN : (cl > 0 ? r_hi : rho);
            rvi[s] = cl < 0 ? 1.0 / RHO_MIN : (cl > 0 ? 1.0 / r_hi : 1.0 / rho);
        }
        __syncthreads();  // every ys / Z read before w is written
#pragma unroll
        for (int s = 0; s < RS; ++s) L.w[ri[s]] = rv[s] * Z[s] - y[s];  // w = rho z_prev - y (rho may be new)
        const int stop_at = run_stop(p, iter);
        __syncthreads();
        PH(5)
        double* const cw = L.cor + w * 32;  // this wave's c_k rows < 8
        double* const tw = L.tv + w * 32;   // this wave's t_j rows < 8
        while (iter < stop_at) {
            ++iter;
            // rhs = sigma x_prev - q + A' (rho z_prev - y), own column
            {
                double av[K], wv[K];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    av[k] = lds_at(cg.e[k] & 0xFFFFu);
                    wv[k] = lds_at(cg.e[k] >> 16);
                }
                double v = sigma * X - Q;
#pragma unroll
                for (int k = 0; k < K; ++k) v += av[k] * wv[k];
                L.rb[pc] = cv ? v : 0.0;
            }
            __syncthreads();
            PH(1)
            // A (both waves): c_k = sum_{j<k} G_kj b_j, rows < 8
            {
                const double* gq = L.gl + rr * S + 4 * ch;
                double bj[NB - 1][4], ga[NP][4];
#pragma unroll
                for (int j = 0; j < NB - 1; ++j)
#pragma unroll
                    for (int e = 0; e < 4; e += 2) ld2(L.rb + j * S + 4 * ch + e, bj[j][e], bj[j][e + 1]);
#pragma unroll
                for (int q = 0; q < NP; ++q)
#pragma unroll
                    for (int e = 0; e < 4; e += 2) ld2(gq + q * 8 * S + e, ga[q][e], ga[q][e + 1]);
#pragma unroll
                for (int k = 1; k < NB; ++k) {
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < k; ++j)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc += ga[k * (k - 1) / 2 + j][e] * bj[j][e];
                    cw[k * 8 + rr] = reduce8(acc);
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            PHL(12)
            // B: own row t_kb[r] = S_kb^{-1}[r] (b_kb + c_kb); recomputed rows < 8 of t_jr
            double t;
            {
                double v[S], cc[8];
#pragma unroll
                for (int c = 0; c < S; c += 2) ld2(L.rb + kb * S + c, v[c], v[c + 1]);
#pragma unroll
                for (int c = 0; c < 8; c += 2) ld2(cw + kb * 8 + c, cc[c], cc[c + 1]);
                double u[8], uc[8];
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                    ld2(L.rb + jr * S + 8 * cq + i, u[i], u[i + 1]);
                    ld2(cw + jr * 8 + i, uc[i], uc[i + 1]);
                }
#pragma unroll
                for (int c = 0; c < 8; ++c) v[c] += cc[c];
                double a[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < S; ++c) a[c & 3] += SB[c] * v[c];
                t = (a[0] + a[1]) + (a[2] + a[3]);
                double a0 = 0.0, a1 = 0.0;
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                    a0 += SR[i] * (cq == 0 ? u[i] + uc[i] : u[i]);
                    a1 += SR[i + 1] * (cq == 0 ? u[i + 1] + uc[i + 1] : u[i + 1]);
                }
                double tr = a0 + a1;
                tr += dpp<0xB1>(tr);
                tr += dpp<0x4E>(tr);  // sum over the quad (the four column chunks)
                tw[jr * 8 + rq] = tr;
                if (r < 8) tw[kb * 8 + r] = t;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            PHL(13)
            // C: x~_kb[r] = t + sum_s G_{pair_s}[q][r] t_{j_s}[q]
            {
                double gv[2][8], tq[2][8];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) gv[s][q] = lds_at(gslot[s] + q * S * 8);
#pragma unroll
                    for (int q = 0; q < 8; q += 2) {
                        lds_at2(tslot[s] + q * 8, tq[s][q], tq[s][q + 1]);
                    }
                }
                double a0 = 0.0, a1 = 0.0;
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int q = 0; q < 8; q += 2) {
                        a0 += gv[s][q] * tq[s][q];
                        a1 += gv[s][q + 1] * tq[s][q + 1];
                    }
                double d = a0 + a1;
                if (w == 0) {  // block 0 (lower half) + its pair (3,0) from the upper half; block 3: t
                    const unsigned lo = (unsigned)__double2loint(d), hi = (unsigned)__double2hiint(d);
                    const auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
                    const auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
                    const double dl0 = __hiloint2double((int)h2[0], (int)l2[0]);  // lower half's partial
                    const double dl1 = __hiloint2double((int)h2[1], (int)l2[1]);  // upper half's partial
                    d = h ? 0.0 : dl0 + dl1;
                }
                const double xn = t + d;
                L.xt[pc] = xn;
                const double xnew = alpha * xn + (1.0 - alpha) * X;
                DX = xnew - X;
                X = xnew;
            }
            __syncthreads();
            PHL(14)
            // z~ = A x~ ; relaxed + projected z ; y ; next w
            {
                double av0[K], xv0[K], av1[K1], xv1[K1], lo[RS], up[RS], zts[RS];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    av0[k] = lds_at(rg0.e[k] & 0xFFFFu);
                    xv0[k] = lds_at(rg0.e[k] >> 16);
                }
#pragma unroll
                for (int k = 0; k < K1; ++k) {
                    av1[k] = lds_at(rg1.e[k] & 0xFFFFu);
                    xv1[k] = lds_at(rg1.e[k] >> 16);
                }
#pragma unroll
                for (int s = 0; s < RS; ++s) {
                    lo[s] = L.lo[ri[s]];
                    up[s] = L.up[ri[s]];
                }
                zts[0] = av0[0] * xv0[0];
#pragma unroll
                for (int k = 1; k < K; ++k) zts[0] += av0[k] * xv0[k];
                zts[1] = av1[0] * xv1[0];
#pragma unroll
                for (int k = 1; k < K1; ++k) zts[1] += av1[k] * xv1[k];
#pragma unroll
                for (int s = 0; s < RS; ++s) {
                    const double zt = zts[s];
                    const double zr = alpha * zt + (1.0 - alpha) * Z[s];
                    const double zn = __builtin_fmin(__builtin_fmax(zr + rvi[s] * y[s], lo[s]), up[s]);
                    const double dd = rv[s] * (zr - zn);
                    Z[s] = zn;
                    dy[s] = dd;
                    y[s] += dd;
                    L.w[ri[s]] = rv[s] * zn - y[s];
                }
            }
            __syncthreads();
            PH(3)
        }
        // run state back to LDS for the out-of-line phases
        C.X[pc] = X;
        L.dx[pc] = DX;
#pragma unroll
        for (int s = 0; s < RS; ++s) { L.ys[ri[s]] = y[s]; C.Z[ri[s]] = Z[s]; C.dY[ri[s]] = dy[s]; }
        __syncthreads();
        PHC(12)
        can_check = p.check_term && (iter % p.check_term == 0);
        const bool do_rho = p.adaptive_rho && p.rho_interval && (iter % p.rho_interval == 0);
        if (!can_check && !do_rho) break;  // max_iter reached
        info_iter = iter;
        bool stop = false;
        {
            // ---- inline update_info + check_termination (OSQP 0.6 update_info,
            // check_termination, is_primal_infeasible, is_dual_infeasible; the same
            // arithmetic as solve_phases.h::update_info_ph / check_termination_ph) on the
            // register-resident gather lists: no dependent global loads, no calls ----
            const bool unscale = p.scaling && !p.scaled_term;
            const unsigned ysbase = lds_addr(L.ys), dYbase = lds_addr(C.dY), dxbase = lds_addr(L.dx);
            double mx[17], sm[2] = {0.0, 0.0}, adx[RS];
#pragma unroll
            for (int k = 0; k < 17; ++k) mx[k] = 0.0;
#pragma unroll
            for (int s = 0; s < RS; ++s) {  // rows: A x, z, the projected delta y, A dx
                const bool ok = tid + s * T2 < m;
                double ax = 0.0, ad = 0.0;
                auto rowdots = [&](const auto& g) __attribute__((always_inline)) {
                    constexpr int KK = std::extent_v<std::remove_reference_t<decltype(g.e)>>;
#pragma unroll
                    for (int k = 0; k < KK; ++k) {
                        const unsigned e = g.e[k], va = e >> 16;
                        const double a = lds_at(e & 0xFFFFu);
                        ax += a * lds_at(va - xbase + Xbase);
                        ad += a * lds_at(va - xbase + dxbase);
                    }
                };
                if (s == 0) rowdots(rg0);
                else rowdots(rg1);
                adx[s] = ad;
                const double zi = Z[s], pr = ax - zi, ei = 1.0 / Ev[s];
                const double lo = L.lo[ri[s]], up = L.up[ri[s]];
                double d = dy[s];
                if (up > OSQP_INFTY * MIN_SCALING) d = (lo < -OSQP_INFTY * MIN_SCALING) ? 0.0 : cmin(d, 0.0);
                else if (lo < -OSQP_INFTY * MIN_SCALING) d = cmax(d, 0.0);
                if (ok) {
                    mx[0] = vmax(mx[0], fabs(ei * pr));
                    mx[2] = vmax(mx[2], fabs(ei * zi));
                    mx[3] = vmax(mx[3], fabs(ei * ax));
                    mx[7] = vmax(mx[7], fabs(pr));
                    mx[9] = vmax(mx[9], fabs(zi));
                    mx[10] = vmax(mx[10], fabs(ax));
                    mx[14] = vmax(mx[14], fabs(unscale ? Ev[s] * d : d));
                    sm[0] += up * cmax(d, 0.0) + lo * cmin(d, 0.0);
                    C.dY[ri[s]] = d;  // projected in place, as OSQP's is_primal_infeasible
                }
            }
            {  // the lane's column: P x, A' y, P dx, and the delta x norm
                double px = 0.0, pdx = 0.0, aty = 0.0;
#pragma unroll
                for (int k = 0; k < KPK; ++k) {
                    const unsigned e = pg.e[k], va = e >> 16;
                    const double pv = lds_at(e & 0xFFFFu);
                    px += pv * lds_at(va);
                    pdx += pv * lds_at(va - Xbase + dxbase);
                }
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const unsigned e = cg.e[k];
                    aty += lds_at(e & 0xFFFFu) * lds_at((e >> 16) - wbase + ysbase);
                }
                if (cv) {
                    const double d = (Q + px) + aty, di = 1.0 / Dv;
                    mx[1] = fabs(di * d);
                    mx[4] = fabs(di * Q);
                    mx[5] = fabs(di * aty);
                    mx[6] = fabs(di * px);
                    mx[8] = fabs(d);
                    mx[11] = fabs(Q);
                    mx[12] = fabs(aty);
                    mx[13] = fabs(px);
                    mx[15] = fabs(unscale ? Dv * DX : DX);
                    mx[16] = fabs(unscale ? pdx * di : pdx);
                }
            }
            // q' dx with the out-of-line phases' column-per-thread order (column tid)
            if (p.pad_var[tid] >= 0) sm[1] = L.qv[tid] * L.dx[tid];
            block_max_sum_tr<T2, 17, 2>(mx, sm, L.red);
            PHC(13)
            Res R;
            if (unscale) {
                R.pri = mx[0]; R.dua = cinv * mx[1];
                R.nz = mx[2]; R.nax = mx[3]; R.nq = mx[4]; R.naty = mx[5]; R.npx = mx[6];
            } else {
                R.pri = mx[7]; R.dua = mx[8];
                R.nz = mx[9]; R.nax = mx[10]; R.nq = mx[11]; R.naty = mx[12]; R.npx = mx[13];
            }
            R.rpri = mx[7]; R.rdua = mx[8]; R.rz = mx[9]; R.rax = mx[10]; R.rq = mx[11]; R.raty = mx[12]; R.rpx = mx[13];
            if (m == 0) R.pri = 0.0;
            if (tid == 0) R.save(L.res);
            if (can_check) {
                int st = MPCQP_UNSOLVED_;
                double obj = 0.0;
                bool done = false;
                if (R.pri > OSQP_INFTY || R.dua > OSQP_INFTY) {
                    st = MPCQP_NON_CVX_;
                    obj = __builtin_nan("");
                    done = true;
                } else {
                    const bool prim_ok = m == 0 || R.pri < p.eps_abs + p.eps_rel * cmax(R.nz, R.nax);
                    double mxd = cmax(cmax(R.nq, R.naty), R.npx);
                    if (unscale) mxd *= cinv;
                    const bool dual_ok = R.dua < p.eps_abs + p.eps_rel * mxd;
                    bool prim_inf = false, dual_inf = false;
                    if (!prim_ok || !dual_ok) {  // infeasibility certificates (uniform branches)
                        // OSQP's is_primal_infeasible / is_dual_infeasible evaluate their tests in
                        // order and return at the first that fails: the reduced norms and sums
                        // decide whether the gathered A'dy maximum / the A dx row test is needed
                        const double norm_dy = mx[14], norm_dx = mx[15], epi = p.eps_pinf, edi = p.eps_dinf;
                        const double cs = unscale ? cval : 1.0;
                        if (!prim_ok && m != 0 && norm_dy > epi && sm[0] < epi * norm_dy) {
                            __syncthreads();  // the projected delta y
                            double na[1] = {0.0};
                            double a = 0.0;
#pragma unroll
                            for (int k = 0; k < K; ++k) {
                                const unsigned e = cg.e[k];
                                a += lds_at(e & 0xFFFFu) * lds_at((e >> 16) - wbase + dYbase);
                            }
                            if (cv) na[0] = fabs(unscale ? a * (1.0 / Dv) : a);
                            block_max<T2, 1>(na, L.red);
                            prim_inf = na[0] < epi * norm_dy;
                        }
                        if (!dual_ok && norm_dx > edi && sm[1] < cs * edi * norm_dx && mx[16] < cs * edi * norm_dx) {
                            bool viol = false;
#pragma unroll
                            for (int s = 0; s < RS; ++s) {
                                if (!(tid + s * T2 < m)) continue;
                                const double ar = unscale ? adx[s] * (1.0 / Ev[s]) : adx[s];
                                const double lo = L.lo[ri[s]], up = L.up[ri[s]];
                                if ((up < OSQP_INFTY * MIN_SCALING && ar > edi * norm_dx) ||
                                    (lo > -OSQP_INFTY * MIN_SCALING && ar < -edi * norm_dx))
                                    viol = true;
                            }
                            dual_inf = !block_any<T2>(viol, L.flag);
                        }
                    }
                    if (prim_ok && dual_ok) {
                        st = MPCQP_SOLVED_;
                        done = true;
                    } else if (prim_inf) {
                        st = MPCQP_PRIMAL_INFEASIBLE_;
                        obj = OSQP_INFTY;
                        if (tid == 0) L.flag[3] = unscale;
                        done = true;
                    } else if (dual_inf) {
                        st = MPCQP_DUAL_INFEASIBLE_;
                        obj = -OSQP_INFTY;
                        if (tid == 0) L.flag[2] = unscale;
                        done = true;
                    }
                }
                __syncthreads();
                if (done && tid == 0) { L.flag[1] = st; L.res[14] = obj; }
                __syncthreads();
                status = done ? st : MPCQP_UNSOLVED_;
                stop = done;
            }
        }
        PHC(14)
        if (!stop && do_rho) {
            // (a rho step with no termination check at this iteration -- check_termination 0, or
            // an interval that is no multiple of it: the check's barriers are the only ones
            // between thread 0's save and this read)
            if (!can_check) __syncthreads();
            Res R;
            R.restore(L.res);
            adapt_rho(p, R, rho, rho_updates, need_factor);
        }
        __syncthreads();
        PH(4)
        if (stop || iter >= p.max_iter) break;
    }
    conclude<T2>(p, b, xo, yo, cval, cinv, rho, status, can_check, iter, info_iter, rho_updates);
#ifdef MPCQP_PHASE_PROF
    if (prof) {
        __syncthreads();
        PH(5)
        if (tid == 0) {
            prof_flush(p, b, L, t0c, t0w, 14);
#ifndef MPCQP_CHECK_PROF
            p.prof[b * kProfSlots + 2] = L.pacc[12] + L.pacc[13] + L.pacc[14];
#endif
        }
    }
#endif
}

// the kernel: the solve, then (last workgroup only) the dispatch order of the next launch
template <int K, int RS, int KPK, int K1>
__global__ __launch_bounds__(T2, 1) void k_solve_w2(KParams p, double* __restrict__ xo, double* __restrict__ yo,
                                                    int factor_only) {
    solve_w2_body<K, RS, KPK, K1>(p, xo, yo, factor_only);
    extern __shared__ __attribute__((aligned(16))) double sm[];
    order_epilogue<T2>(p, (int*)sm);
}

// Fused setup + solve (mpcqp_setup_solve_device): the workgroup Ruiz-scales its
// instance with the register-list setup (setup_r.h, the same arithmetic as k_setup /
// k_setup_r), then solves it.  Everything the solve reads from the workspace was
// written by this workgroup before the barrier, so no second kernel, no launch gap and
// no setup kernel in front of the slowest instance.
template <int K, int RS, int KPK, int K1, int SK, int SRS, int SAS, int SPS>
__global__ __launch_bounds__(T2, 1) void k_setup_solve_w2(KParams p, const double* __restrict__ Px_in,
                                                          const double* __restrict__ Ax_in,
                                                          const double* __restrict__ q_in,
                                                          const double* __restrict__ l_in,
                                                          const double* __restrict__ u_in, double* __restrict__ xo,
                                                          double* __restrict__ yo) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    setup_r_body<T2, SK, 4, SRS, SAS, SPS>(p, instance_of(p), Px_in, Ax_in, q_in, l_in, u_in, sm);
    __syncthreads();
    solve_w2_body<K, RS, KPK, K1>(p, xo, yo, 0);
    order_epilogue<T2>(p, (int*)sm);
}

// ---------------------------------------------------------------------------
// Four-wave variant (variant 17, k_solve_w4 / k_setup_solve_w4): one 256-thread
// workgroup per QP, wave k owns block k.  Lane (h, r) keeps row r of S_k^{-1}, columns
// [16 h, 16 h + 16) (32 VGPRs instead of the two-wave kernel's 64 + 16), and row i = tid
// of A.  Per iteration:
//   rhs   column k S + r (both halves compute it, the lower half stores)   -> barrier
//   A     c_k = sum_{j<k} G_kj b_j, rows < 8 (wave k only its own block)  -> wave sync
//   B     t_k[r] = S_k^{-1}[r] (b_k + c_k): half-row sums + permlane32     -> barrier
//   C     x~_k[r] = t_k[r] + sum_{j>k} G_jk' t_j[0, 8): the pairs split over the halves
//   rows  z~ = A x~ (one row per lane), relaxation, projection, y, w      -> barrier
// Four barriers instead of three, but each wave issues about 60 % of a two-wave wave's
// instructions, and the factorisation pre-pivots the four blocks at once
// (solve_phases.h::factorize_w4).  Operands that do not change within a run (the row's
// and half-column's A values, the row bounds, phase A's and phase C's G values) are
// loaded into registers at the run start: fewer LDS reads (and waits) per iteration on
// every wave's path.  MPCQP_VARIANT=17 (A/B against variant 10).
constexpr int T4 = 256;

// EL: the plan has eliminated columns (plan.h Plan::eown; the slack layouts).  The upper
// half-wave lane (1, r) of wave w then owns the eliminated column pe = eown[w S + r] of its
// block column's variable: it folds -ec b_pe into its half of the block column's rhs sum
// (b_p - (K_pj / K_jj) b_j, no extra exchange), keeps x_pe, q_pe and b_pe in its registers,
// and after phase C sets  x~_pe = ed b_pe - ec x~_p  (ed = 1 / K_jj, ec = K_pj / K_jj,
// factorize_w4) -- the elementwise back-substitution of the scalar Schur complement --
// which the rows phase reads from xt like any other column.  Its termination-check column
// is pe (the lower half keeps the block column).
// DK (dense inverse, no eliminated columns): the three-phase solve x~ = L' D L b (L = I + the
// G blocks below the diagonal, D = diag(S_k^{-1}); phases A, B, C above) replaced by one
// product with M^{-1} = L' D L formed explicitly after each factorisation.  Lane (h, r) of
// wave a keeps row a S + r of M^{-1} over the real columns of blocks 2 h and 2 h + 1 (the
// first NBC of each: plan.cpp's balanced merge keeps every block at <= NBC real columns):
//   rhs   -> barrier ->   x~ = M^{-1} b: 2 NBC FMAs per lane, one permlane32   -> barrier -> rows
// Three barriers a step instead of four, and no phase whose length depends on the block
// (the three-phase form's wave 3 runs three phase-A pairs, wave 0 two phase-C slots).
// Block (a, b) of L' D L is  sum over k >= max(a, b) of  L_ka' S_k^{-1} L_kb  (L_kk = I, L_kj
// = G_kj for j < k, nonzero rows < QR):
//   [a = b] S_a^{-1}[i][c]
//   + sum_q S_a^{-1}[i][q] G_ab[q][c]                       (a > b)
//   + sum_q G_ba[q][i] S_b^{-1}[q][c]                       (b > a)
//   + sum_{k > a, k > b} sum_q V_ka[i][q] G_kb[q][c],  V_ka[i][q] = sum_p G_ka[p][i] S_k^{-1}[p][q]
// Each term is a sum of rank-one row updates: a lane coefficient times a row read from LDS
// by broadcast (one row per half-wave).  G blocks come from the LDS copy gl (pair (k, j) at
// k (k - 1) / 2 + j, pair NP the zero block: a lane whose b does not satisfy the term's
// condition reads zeros), S_k^{-1} from the LDS tiles Sg.
// M^{-1} = L' D L into the instance's Kd rows, in 4 x 8 tiles: wave a forms block row a,
// lanes [16 b, 16 b + 16) block (a, b), lane l16 = lane & 15 the rows 4 (l16 >> 1) .. + 3 and
// columns 16 (l16 & 1) .. + 15 in two passes of 8 -- an outer-product update per term step
// (4 coefficients, 8 row values, 32 FMAs) instead of a 28-wide row per lane (28 values for 28
// FMAs): 3/8 of the LDS reads per FMA, the wave's steps 5 [a > 0] + 5 [a < 3] + 5 (3 - a) (pair NP, the
// zero block, for the blocks a term does not apply to).  Element (i, c) of block (a, b) goes
// to the dense-row slot of its lane (a, b & 1, i): pair j / 2 of the lane's row, j = c (b < 2)
// or NB0 + c (b >= 2), c below NB0 / NB1 only.  Stored through global memory, read back by
// other lanes after the next workgroup barrier.
template <int QR, int NB0, int NB1>
__device__ __forceinline__ void form_dense_rows(__attribute__((address_space(1))) dpair* kd, const double* Sg,
                                                const double* gl, int a, int lane) {
    constexpr int NP = 6, T4_ = 256, TC = 8;  // TC: tile columns per pass (two passes of the lane's 16)
    auto pidx = [](int x, int y) { return y < x ? x * (x - 1) / 2 + y : NP; };
    const int bq = lane >> 4, l16 = lane & 15, i0 = 4 * (l16 >> 1);
    const double* const Ta = Sg + a * SS;
    const int nbs = (bq >> 1) ? NB1 : NB0, jb = (bq >> 1) ? NB0 : 0;
    const unsigned t0 = (unsigned)(a * 64 + (bq & 1) * 32 + i0);
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        const int c0 = 16 * (l16 & 1) + TC * pass;
        double acc[4][TC];
        {   // [a = b] the tile of S_a^{-1}
            const double* src = Sg + bq * SS + i0 * S + c0;
            const bool diag = bq == a;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < TC; c += 2) {
                    double v0, v1;
                    ld2(src + i * S + c, v0, v1);
                    acc[i][c] = diag ? v0 : 0.0;
                    acc[i][c + 1] = diag ? v1 : 0.0;
                }
        }
        auto step = [&](const double (&cf)[4], const double* row) __attribute__((always_inline)) {
            double rv[TC];
#pragma unroll
            for (int c = 0; c < TC; c += 2) ld2(row + c, rv[c], rv[c + 1]);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < TC; ++c) acc[i][c] += cf[i] * rv[c];
        };
        if (a > 0) {  // (a > b): S_a^{-1}[i][q] G_ab[q][c]
            const double* g = gl + pidx(a, bq) * 8 * S + c0;
#pragma unroll
            for (int q = 0; q < QR; ++q) {
                double cf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) cf[i] = Ta[(i0 + i) * S + q];
                step(cf, g + q * S);
            }
        }
        if (a < 3) {  // (b > a): G_ba[q][i] S_b^{-1}[q][c]
            const double* g = gl + pidx(bq, a) * 8 * S + i0;
            const double* Tb = Sg + bq * SS + c0;
#pragma unroll
            for (int q = 0; q < QR; ++q) {
                double cf[4];
                ld2(g + q * S, cf[0], cf[1]);
                ld2(g + q * S + 2, cf[2], cf[3]);
                step(cf, Tb + q * S);
            }
        }
#pragma unroll 1
        for (int k = a + 1; k < 4; ++k) {  // (k > a, k > b): V_ka[i][q] G_kb[q][c]
            const double* gka = gl + pidx(k, a) * 8 * S + i0;
            const double* gkb = gl + pidx(k, bq) * 8 * S + c0;
            const double* Tk = Sg + k * SS;
            double V[4][QR];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int q = 0; q < QR; ++q) V[i][q] = 0.0;
#pragma unroll
            for (int pp = 0; pp < QR; ++pp) {
                double g[4];
                ld2(gka + pp * S, g[0], g[1]);
                ld2(gka + pp * S + 2, g[2], g[3]);
#pragma unroll
                for (int q = 0; q < QR; ++q) {
                    const double t = Tk[pp * S + q];
#pragma unroll
                    for (int i = 0; i < 4; ++i) V[i][q] += g[i] * t;
                }
            }
#pragma unroll
            for (int q = 0; q < QR; ++q) {
                const double cf[4] = {V[0][q], V[1][q], V[2][q], V[3][q]};
                step(cf, gkb + q * S);
            }
        }
        // element (i0 + i, c0 + c) -> lane a 64 + (bq & 1) 32 + i0 + i, pair (jb + c0 + c) / 2
#pragma unroll
        for (int c = 0; c < TC; c += 2) {
            if (c0 + c < nbs) {
                const unsigned jp = (unsigned)((jb + c0 + c) >> 1);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    kd[jp * T4_ + t0 + i].x = acc[i][c];
                    kd[jp * T4_ + t0 + i].y = acc[i][c + 1];
                }
            }
        }
    }
}

// K: row-list length, KC: column-list length (even: the rhs splits it over the half-waves).
// factor_only: return after the first factorisation (the setup-time convexity check of
// api.hip::check_convex); the fused setup + solve kernel passes 0
// RU (the stand-alone solve kernel, k_solve_w4, not the fused setup + solve): the first
// factorisation of a solve takes setup()'s convexity factor when it is current (KParams::ffresh:
// the factor-only launch leaves the S_k^{-1} tiles in the instance's Si region, the G blocks in H
// and the eliminated columns' ec / ed in F); the factor-only launch (factor_only) persists them
// ONE (the one-shot fused kernel, mpcqp_set_one_shot; cold start): the setup left the scaled
// problem in this carve (setup_r.h ONE) and finalize stores no warm-start state -- no workspace
// round trip for data no later call reads; GL 1 (where the LDS budget of two workgroups per CU
// allows it, one_shot_form 2): the G blocks go to an LDS region after the S_k^{-1} tiles instead
// of the instance's H tiles, a refactorisation keeps y there instead of in the workspace, and
// the setup leaves E and D in the carve (edl_E / edl_D); GL 2 (one_shot_form 3): the G blocks go
// straight into gl (factorize_w4_gl); GL 3 (form 2 without eliminated columns and amax <= 5, the
// headline's plan): GL 1 with the loop's phase A and B reads issued earlier (WV below) and the
// Gauss-Jordan pivot's reciprocal taken off its LDS round trip (factorize_gp_nl) -- the same sums
// and operands; GL 4 (the same plan, the default there): GL 3 with the run's loop compiled once
// per wave role (admm_run<W>, solve_w4_run.inc) -- what serves the other waves' roles leaves each
// wave's path, the arithmetic stays operand for operand; GL 5 (that plan with amax = bmax = 5, the
// default there): GL 4 with the factorisation compiled for those constants and per wave role
// (factorize_gq_nl) -- the same sums; GL 1, GL 3 and GL 4 stay as the A/B baselines
// (MPCQP_ONE_SHOT_LOOP=lds / wave / roles) and keep their code
template <int K, int KPK, int QR, bool EL = false, int KC = K, bool DK = false, bool RU = false, bool ONE = false,
          int GL = 0>
__device__ __forceinline__ void solve_w4_body(const KParams& p, double* __restrict__ xo, double* __restrict__ yo,
                                              int factor_only = 0) {
    static_assert(!(DK && EL), "the dense inverse covers plans without eliminated columns");
    const int tid = threadIdx.x, w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int h = lane >> 5, r = lane & 31;  // (rr, ch: per pass, below)
    constexpr int NB = 4, NP = NB * (NB - 1) / 2;  // exactly four blocks (solve.hip::variant_fits)
    static_assert(KC % 2 == 0, "the rhs splits the column list over the half-waves");
    constexpr int KH = KC / 2;                       // column-list entries per half in the rhs
    constexpr int LE = 2;                           // A entries of an eliminated column (plan ecnt <= 2)
    const long b = instance_of(p);
    const int n = p.n, m = p.m, npad = p.npad, nnzP = p.nnzP, nnzA = p.nnzA;
    SL2 C = carve(p);
    SLds& L = C.L;
    static_assert(GL >= 0 && GL <= 5 && (GL < 3 || (ONE && !EL && !DK && QR <= 5)), "GL 3, 4, 5: the headline's plan");
    constexpr bool G1 = GL == 1 || GL >= 3;  // the one-shot form 2 (G blocks, y, E and D on chip)
    constexpr bool WV = GL >= 3;             // ... with the loop's phase A / B reads issued earlier
    constexpr bool ROLES = GL >= 4;          // ... and the run's loop compiled once per wave (admm_run)
    // GL 1: the G blocks (amax x S per pair) go to LDS after the S_k^{-1} tiles; GL 2: straight
    // into gl (factorize_w4_gl), no copy
    const double* Hg = G1 ? w4_tiles(p, C) + (long)NB * SS : p.H + b * (long)p.nb * SS;
    double* const Sg = w4_tiles(p, C);  // S_k^{-1} tiles in LDS (lds_w2_bytes)
    // SWZ: the tiles in tile_at<true>'s layout (solve_phases.h) -- the one-shot form 2 without
    // eliminated columns and amax <= 5, the headline's instantiation.  Its tiles never leave LDS
    // (no RU / factor_only copy, no dense rows); the other instantiations' stay row-major
    constexpr bool SWZ = ONE && G1 && !EL && !DK && QR <= 5;
    // LEAN (the same instantiation): the work between its ADMM runs cut to what the result needs
    // -- the run start reads the G blocks where the factorisation left them (no gl copy) and
    // divides once, the check takes its column list from the run's registers and combines the
    // waves' maxima a lane each (block_max_sum_tr's LANE), and the rho step keeps the check's
    // residuals in registers.  Every floating-point operation, operand and order is the
    // general code's
    constexpr bool LEAN = SWZ;

    if (p.err[b]) {
        reject_instance<T4>(p, b, xo, yo);
        return;
    }
    PROF_START
    // OPQ: the instantiations whose solve loop leaves no register for values used only at run
    // starts, refactorisations and checks (the eliminated-column and QR = 8 ones); they form
    // those values where used (see the lane identity at the top of the outer loop)
    constexpr bool OPQ = EL || QR > 5;
    // c and 1 / c of the cost scaling, from the instance's scal slots where used
    // (ROLES: from the copy in L.cor made below -- a check reads them without a global round trip)
    constexpr int kCorScal = 40;  // the copy's slots: L.cor[40], L.cor[41]
    auto cscal = [&](int k) __attribute__((always_inline)) {
        if constexpr (ROLES) return L.cor[kCorScal + k];
        return OPQ ? opaque_gptr(p.scal + b * 4)[k] : p.scal[b * 4 + k];
    };
    double rho = p.scal[b * 4 + 2];
    const double sigma = p.sigma, alpha = p.alpha;
    const bool warm = !ONE && p.warm_start != 0;
    const int mp = solve_mpad(m);
    if constexpr (!ONE) {
        // (load_instance's text: the call cost k_solve_w4 two spilled SGPRs without eliminated
        // columns and moved four with them)
        for (int e = tid; e < nnzA; e += T4) L.Acsc[e] = p.Ax[b * nnzA + e];
        if (tid == 0) L.Acsc[nnzA] = 0.0;
        for (int v = tid; v < nnzP; v += T4) L.Pv[v] = p.Px[b * nnzP + v];
        if (tid == 0) L.Pv[nnzP] = 0.0;
        for (int i = tid; i < mp; i += T4) {
            const bool in = i < m;
            L.lo[i] = in ? p.l[b * m + i] : 0.0;
            L.up[i] = in ? p.u[b * m + i] : 0.0;
            L.ct[i] = in ? p.ct[b * m + i] : 0;
            C.Z[i] = (in && warm) ? p.z[b * m + i] : 0.0;
        }
        for (int pc = tid; pc < npad; pc += T4) {
            L.qv[pc] = p.q[b * npad + pc];
            C.X[pc] = warm ? p.x[b * npad + pc] : 0.0;
        }
    } else {
        if (tid == 0) L.Acsc[nnzA] = 0.0;
        if (tid == 0) L.Pv[nnzP] = 0.0;
        if constexpr (GL == 2)  // (factorize_w4_gl writes rows < amax of the pairs; the rest stays zero)
            for (int o = tid; o < (NP + 1) * 8 * S; o += T4) L.gl[o] = 0.0;
    }
    if (tid < 8) L.cor[tid] = 0.0;        // c_0 = 0 (block 0 has no correction)
    if (tid < 8) L.cor[32 + tid] = 0.0;   // the upper half's zero correction row (phase B)
    if (tid < 16) L.res[tid] = 0.0;
    if (tid < 4) L.flag[tid] = 0;
    // ROLES: c and 1 / c of the cost scaling, which every check took from global memory, kept on
    // chip from here on in two slots of L.cor that the four-wave kernel leaves unused (it holds
    // nb S doubles; the loop uses [0, 40): c_w and the zero row).  The first pass's opening
    // barrier orders them before any read
    if constexpr (ROLES) {
        static_assert(kCorScal + 2 <= NB * S, "the carve's unused L.cor slots");
        if (tid < 2) L.cor[kCorScal + tid] = p.scal[b * 4 + tid];
    }

    int status = MPCQP_UNSOLVED_, rho_updates = 0, iter = 0, info_iter = 0;
    bool can_check = false, need_factor = true;
    const bool low = h == 0;
    const int pe0 = (EL && !low) ? p.eown[w * S + r] : -1;  // the upper lane's eliminated column, or -1
    const bool colv = low && p.pad_var[w * S + r] >= 0;     // a real block column (padding: rb = 0)
    // (ROLES: the check's "column tid is a real one", held from here instead of loaded per check;
    // kept per column in LDS instead it spilled two VGPRs)
    [[maybe_unused]] const bool padme = ROLES && tid < npad && p.pad_var[ROLES ? tid : 0] >= 0;
    double* const Fo = p.F + b * (long)p.nb * SS;    // ec, ed of the eliminated columns (factorize_w4)
    double ec = 0.0, ed = 0.0;
    const unsigned abase = lds_addr(L.Acsc), wbase = lds_addr(L.w), xbase = lds_addr(L.xt);
    const unsigned Xbase = lds_addr(C.X);
    GatherW<K> rg;
    GatherW<KH> chs;  // the half's share of the block column's list (the rhs sums)
    GatherW<LE> el;   // EL: the eliminated column's list (zero entries for the other lanes)
    const bool rows_wave = w * 64 < mp;  // wave-uniform
    // DK: the lane's half of row pc of M^{-1}: columns [0, NB0) of block h and [0, NB1) of block
    // 2 + h (their real columns), formed after each factorisation.  NB0 = 26, NB1 = 28
    // (dense_w4: bsize[0], bsize[1] <= 26 and bsize[2], bsize[3] <= 28; cfg 2's balanced
    // blocks are 26 / 25 / 25 / 28)
    constexpr int NB0 = 26, NB1 = 28;
    static_assert(!DK || (NB0 + NB1) * T4 == kDenseRowDoubles, "KParams::Kd rows");
    double Kr[DK ? NB0 + NB1 : 1];
    constexpr int DKW = 8;  // DK: b values read per batch of the product (even)
    PH(5)
    for (;;) {
        // The lane's identity through an empty asm at each pass (opaque_v): the addresses and
        // slot offsets that a refactorisation, the run start and a check form from it are
        // formed in the pass, instead of once per kernel and then held -- spilled to scratch
        // -- across the solve.  Only where the solve loop leaves no register for them (the
        // eliminated-column and QR = 8 instantiations: 42 and 17 spilled values without it,
        // none with it, cfg 3 45.5 -> 44.0 ms); the cfg-2 kernel (QR = 5) spills nothing
        // either way and is 1 % faster keeping them (same-box A/B 0.433 vs 0.439 ms).
        const int tid = OPQ ? opaque_v(threadIdx.x) : (int)threadIdx.x;
        const int lane = tid & 63, h = lane >> 5, r = lane & 31, rr = lane >> 3, ch = lane & 7;
        const int pc = w * S + r;  // the lane's column (both halves; the lower half stores)
        const int pe = OPQ ? opaque_v(pe0) : pe0;
        const int xc = pe >= 0 ? pe : pc;  // the column whose x, q the lane keeps
        const int ri = min(tid, mp - 1);   // lanes past the padded rows repeat the inert last row
        __syncthreads();
        if (need_factor) {
            need_factor = false;
            if (iter > 0) {
                if constexpr (G1) {  // (y kept on chip, after the G blocks)
                    double* const ysv = Sg + (long)NB * SS + (long)(NB * (NB - 1) / 2) * p.amax * S;
                    for (int i = tid; i < m; i += T4) ysv[i] = L.ys[i];
                } else {
                    const auto yp = opaque_gptr(p.y + b * m);
                    for (int i = tid; i < m; i += T4) yp[i] = L.ys[i];
                }
                __syncthreads();  // every ys read is done before factorize_w4's E tiles overwrite it
            }
            // the slack layouts' (EL) factorisation with rotated tile rows: cfg 3
            // 43.38 -> 43.16 ms; cfg 2's build lost 1.6 % to the register assignment it moved
            // (profiles/r3s3_ab/ab_swz*.json)
            bool ok;
            if constexpr (RU) {
                // the workspace factor is setup()'s (same data, rho and row classes: the same
                // arithmetic, so the same tiles) -- used once: this solve's later factorisations,
                // and the ones of later solves, are its own
                if (iter == 0 && p.reuse && p.ffresh[b] == 1 && p.scal[b * 4 + 3] == rho) {
                    const double2* src = (const double2*)(p.Si + b * (long)p.nb * SS);
                    for (int e = tid; e < 2 * SS; e += T4) ((double2*)Sg)[e] = src[e];
                    ok = true;
                } else if constexpr (EL) {
                    ok = factorize_lds_nl<T4, EL>(p.self, b, rho);
                } else {
                    ok = factorize_nl<T4, EL>(p.self, b, rho, Sg);
                }
                __syncthreads();
                if (tid == 0) p.ffresh[b] = 0;
            } else if constexpr (GL == 5) {  // (amax = bmax = 5: factorize_w4q)
                ok = factorize_gq_nl<T4, SWZ, 5, 5>(p.self, b, rho);
            } else if constexpr (WV) {  // (the Gauss-Jordan pivot in registers: gj_seg SEG 3 / 4)
                ok = factorize_gp_nl<T4, EL, SWZ>(p.self, b, rho);
            } else if constexpr (G1) {
                ok = factorize_g_nl<T4, EL, SWZ>(p.self, b, rho);
            } else if constexpr (GL == 2) {
                ok = factorize_gl_nl<T4, EL>(p.self, b, rho);
            } else if constexpr (EL) {
                // (the tiles from the carve: an LDS-typed pointer, ds_ accesses -- cfg 3's
                // factorisation was compiled with flat ones)
                ok = factorize_lds_nl<T4, EL>(p.self, b, rho);
            } else {
                ok = factorize_nl<T4, EL>(p.self, b, rho, Sg);
            }
            if (!ok) {
                if (iter == 0) {
                    // (reject_instance's stores through opaque_ptr, on purpose: with the plain
                    // ones the eliminated-column instantiations' ADMM loop changes)
                    if (xo) for (int j = tid; j < n; j += T4) opaque_ptr(xo + b * n)[j] = __builtin_nan("");
                    if (yo) for (int i = tid; i < m; i += T4) opaque_ptr(yo + b * m)[i] = __builtin_nan("");
                    if (tid == 0) fail_status(p, b);
                    return;
                }
                status = MPCQP_NON_CVX_;
                can_check = true;
                break;
            }
            if (factor_only) {  // (setup()'s convexity check: its tiles for the first solve, RU)
                __syncthreads();
                double2* dst = (double2*)(p.Si + b * (long)p.nb * SS);
                for (int e = tid; e < 2 * SS; e += T4) dst[e] = ((const double2*)Sg)[e];
                if (tid == 0) {
                    p.ffresh[b] = 1;
                    p.scal[b * 4 + 3] = rho;  // the factor's rho (the RU solve checks it against scal[2])
                }
                return;
            }
            __syncthreads();
            const bool have_y = iter > 0 || warm;
            if constexpr (G1) {
                const double* const ysv = Sg + (long)NB * SS + (long)(NB * (NB - 1) / 2) * p.amax * S;
                for (int i = tid; i < mp; i += T4) L.ys[i] = (have_y && i < m) ? ysv[i] : 0.0;
            } else {
                const auto yp = opaque_gptr(p.y + b * m);
                for (int i = tid; i < mp; i += T4) L.ys[i] = (have_y && i < m) ? yp[i] : 0.0;
            }
            if constexpr (GL != 2 && !LEAN) {  // (LEAN: the run start reads the blocks at Hg)
                for (int o = tid; o < (NP + 1) * 8 * S; o += T4) {
                    const int q = o >> 8, t = (o >> 5) & 7;
                    L.gl[o] = (q < NP && t < p.amax) ? Hg[(long)q * p.amax * S + (o & 255)] : 0.0;
                }
            }
            chs.load(p.gcol + (h ? KH : 0) * npad + pc, npad, abase, wbase);
            if constexpr (EL) {
                if (pe >= 0) {
                    el.load(p.gcol + pe, npad, abase, wbase);
                    const int e = pe - p.nb * S;
                    ec = Fo[2 * e];
                    ed = Fo[2 * e + 1];
                } else {
                    el.clear(abase + 8u * nnzA, wbase);
                }
            }
            if (ri < m) rg.load(p.grow + ri, m, abase, xbase);  // by ri: duplicate lanes repeat its row
            else rg.clear(abase + 8u * nnzA, xbase);
            if constexpr (DK) {
                // M^{-1}'s rows formed once per factorisation and kept in the instance's Kd rows
                // (lane-contiguous pairs): each run start reloads them, so that nothing lives in
                // registers across the termination check -- the check's registers and the
                // 108 of the rows do not fit together (spilled, and wrong in the divergent
                // check: DESIGN.md §5)
                __syncthreads();  // the G copy is complete
                // (the instance's base through an empty asm, the lanes' 32-bit indices formed at
                // the stores; the run start's reads follow a workgroup barrier)
                form_dense_rows<QR, NB0, NB1>((__attribute__((address_space(1))) dpair*)opaque_gptr(
                                                  p.Kd + b * kDenseRowDoubles),
                                              Sg, L.gl, w, lane);
                __syncthreads();  // every tile stored before any lane reads its rows (run start)
            }
            PH(0)
        }
        // ---- run state ----
        if constexpr (DK) {
            const auto kd = (const __attribute__((address_space(1))) dpair*)opaque_gptr(p.Kd + b * kDenseRowDoubles);
#pragma unroll
            for (int j = 0; j < NB0 + NB1; j += 2) {
                Kr[j] = kd[(unsigned)((j / 2) * T4 + tid)].x;
                Kr[j + 1] = kd[(unsigned)((j / 2) * T4 + tid)].y;
            }
        }
        double SB[16];
        if constexpr (SWZ) {
            // (the row through an empty asm: the eight swizzled positions are formed here, at the
            // run start, instead of once per kernel and then held across the solve -- 2 spilled
            // VGPRs that way)
            const double* src = Sg + (long)w * SS;
            const int rs = opaque_v(r);
#pragma unroll
            for (int c = 0; c < 16; c += 2) ld2(src + tile_at<true>(rs, 16 * h + c), SB[c], SB[c + 1]);
        } else if constexpr (!DK) {
            const double* src = Sg + (long)w * SS + r * S + 16 * h;
#pragma unroll
            for (int c = 0; c < 16; c += 2) ld2(src + c, SB[c], SB[c + 1]);
        }
        double X = C.X[xc], DX = 0.0;
        const double Q = L.qv[xc];
        // phase-C slots: pairs (j, w), j > w, split over the halves; pair NP is zero
        int gslot[2], tslot[2];
        bool gz[2];  // (LEAN) the slot's pair is the zero pair
        {
            int pr[2] = {NP, NP}, jj[2] = {3, 3};
            if (w == 0) {
                if (h == 0) { pr[0] = 0; jj[0] = 1; pr[1] = 1; jj[1] = 2; }
                else        { pr[0] = 3; jj[0] = 3; }
            } else if (w == 1) {
                if (h == 0) { pr[0] = 2; jj[0] = 2; }
                else        { pr[0] = 4; jj[0] = 3; }
            } else if (w == 2) {
                if (h == 0) { pr[0] = 5; jj[0] = 3; }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                // (LEAN: column r of the pair's block at Hg, amax rows; the zero pair's lanes
                // read pair 0 and take zeros below)
                gslot[s] = LEAN ? lds_addr(Hg + (pr[s] < NP ? pr[s] : 0) * p.amax * S + r)
                                : lds_addr(L.gl + pr[s] * 8 * S + r);
                gz[s] = pr[s] == NP;
                tslot[s] = lds_addr(L.tv + jj[s] * 8);
            }
        }
        const int nsw = (NB - w) >> 1;  // phase-C slots of the wave (wave 0: 2, waves 1-2: 1, wave 3: 0)
        // the half's share of the column list (KH entries; the list is zero-padded to K)
        const GatherW<KH>& ch2 = chs;
        double ca[KH];  // the half's A values of the column (registers for the run)
#pragma unroll
        for (int k = 0; k < KH; ++k) ca[k] = lds_at(ch2.e[k] & 0xFFFFu);
        double ea[LE];  // EL: the eliminated column's A values (zeros on the other lanes)
#pragma unroll
        for (int k = 0; k < LE; ++k) ea[k] = EL ? lds_at(el.e[k] & 0xFFFFu) : 0.0;
        double bj = 0.0;  // EL: b of the eliminated column, from the rhs to phase C
        const double r_hi = RHO_EQ_OVER_RHO_INEQ * rho;
        double y = L.ys[ri], Z = C.Z[ri], dy = 0.0;
        // the row's A values and bounds stay in registers for the run (fewer LDS reads per
        // iteration)
        double av[K];
#pragma unroll
        for (int k = 0; k < K; ++k) av[k] = DK ? 0.0 : lds_at(rg.e[k] & 0xFFFFu);
        const double rlo = L.lo[ri], rup = L.up[ri];
        const signed char cl = L.ct[ri];
        const double rv = cl < 0 ? RHO_MIN : (cl > 0 ? r_hi : rho);
        // (LEAN: one division, of the class's own rv -- the operands of the one selected below)
        const double rvi = LEAN ? 1.0 / rv : (cl < 0 ? 1.0 / RHO_MIN : (cl > 0 ? 1.0 / r_hi : 1.0 / rho));
        __syncthreads();  // (the G copy of a refactorisation is complete)
        // phase A's G values (rows rr < 8 of G_wj, columns [4 ch, 4 ch + 4), j < w) in registers for the run
        double ga[NB - 1][4];
        if constexpr (LEAN) {
            // rows rr < amax at Hg (pair stride amax S: the factorisation's own layout, after
            // its closing barrier); the copy's zero rows are constants
            const int gs = p.amax * S * 8;
            const unsigned gq = lds_addr(Hg) + (w * (w - 1) / 2) * gs + (rr * S + 4 * ch) * 8;
#pragma unroll
            for (int j = 0; j < NB - 1; ++j) {
                ga[j][0] = ga[j][1] = ga[j][2] = ga[j][3] = 0.0;
                if (j < w && rr < p.amax) {
                    lds_at2(gq + j * gs, ga[j][0], ga[j][1]);
                    lds_at2(gq + j * gs + 16, ga[j][2], ga[j][3]);
                }
            }
        } else if constexpr (!DK) {
            const double* gq = L.gl + (w * (w - 1) / 2) * 8 * S + rr * S + 4 * ch;
#pragma unroll
            for (int j = 0; j < NB - 1; ++j) {
                if (j < w) {
                    ld2(gq + j * 8 * S, ga[j][0], ga[j][1]);
                    ld2(gq + j * 8 * S + 2, ga[j][2], ga[j][3]);
                } else {
                    ga[j][0] = ga[j][1] = ga[j][2] = ga[j][3] = 0.0;
                }
            }
        }
        // phase C's G values (column r of the slots' pairs, rows < QR) in registers for the run
        double gc[2][QR];
        if constexpr (LEAN) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int q = 0; q < QR; ++q)
                    gc[s][q] = (s < nsw && !gz[s] && q < p.amax) ? lds_at(gslot[s] + q * S * 8) : 0.0;
        } else if constexpr (!DK) {
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int q = 0; q < QR; ++q) gc[s][q] = s < nsw ? lds_at(gslot[s] + q * S * 8) : 0.0;
        }
        if (rows_wave) L.w[ri] = rv * Z - y;  // (lanes past the padded rows may hold a stale y)
        const int stop_at = run_stop(p, iter);
        __syncthreads();
        PH(15)  // (the run starts; slot 5 keeps the kernel's start and finalize)
        // The run's loop (solve_w4_run.inc: the text between here and the write-back).  ROLES
        // compiles it once per wave role: admm_run<W> re-forms the wave's index and what follows
        // from it alone (nsw, the wave's column) from the compile-time W and is reached once per
        // run through a switch on w.  With W a constant the tests that are uniform within a
        // wave fold: the selects, zero-fills and moves that serve the other roles leave the
        // wave's path, and so does arithmetic whose result the role never stores (wave 0's
        // reduce8).  No operation that reaches x, y, z, w, rb, tv or xt is removed or reordered
        // by hand: what folds is control flow on compile-time constants.  Every
        // other instantiation takes the same text with the run-time w, in place and not through
        // the lambda: going through it with "W = -1" moved the code of all seventeen
        if constexpr (ROLES) {
            auto admm_run = [&](auto wc) __attribute__((always_inline)) {
                constexpr int W = decltype(wc)::value;
                // (rows_wave stays the body's: it depends on the run-time mp, and one copy per
                // role, each live across the kernel, spilled one role's mask: two v_readlane in
                // that role's loop)
                const int w = W, nsw = (NB - W) >> 1, pc = W * S + r;
#include "solve_w4_run.inc"
            };
            switch (w) {
                case 0: admm_run(std::integral_constant<int, 0>{}); break;
                case 1: admm_run(std::integral_constant<int, 1>{}); break;
                case 2: admm_run(std::integral_constant<int, 2>{}); break;
                default: admm_run(std::integral_constant<int, 3>{}); break;
            }
        } else {
#include "solve_w4_run.inc"
        }
        // run state back to LDS (lds_put: the addresses are formed here, not held across the
        // loop)
        if (low) { lds_put(C.X, pc, X); lds_put(L.dx, pc, DX); }
        if (EL && pe >= 0) { lds_put(C.X, pe, X); lds_put(L.dx, pe, DX); }
        if (rows_wave) { lds_put(L.ys, ri, y); lds_put(C.Z, ri, Z); lds_put(C.dY, ri, dy); }
        __syncthreads();
        can_check = p.check_term && (iter % p.check_term == 0);
        const bool do_rho = p.adaptive_rho && p.rho_interval && (iter % p.rho_interval == 0);
        if (!can_check && !do_rho) break;
        info_iter = iter;
        bool stop = false;
        Res Rk;  // (LEAN) the check's residuals, for the rho step
        {
            // the check's per-lane operands come from the plan (shared by every instance: L2
            // hits) and the workspace here, not from registers held through the run: the lane's
            // column (EL: the upper half checks its eliminated column pe) with its A and P lists
            // and D, the row's E
            const int col = EL ? (low ? pc : pe) : pc;
            // (LEAN: col is pc, so cv is the run's colv and the column list is the run's own chs:
            // half h holds entries [h KH, h KH + KH) in the same encoding, and one permlane32
            // swap gives every lane both halves' -- no global load at the head of the check)
            const bool cv = LEAN ? colv : col >= 0 && (EL || low) && opaque_gptr(p.pad_var)[col] >= 0;
            GatherW<KC> cg;
            GatherW<KPK> pg;
            if constexpr (LEAN) {
#pragma unroll
                for (int k = 0; k < KH; ++k) {
                    const auto e2 = __builtin_amdgcn_permlane32_swap(chs.e[k], chs.e[k], false, false);
                    cg.e[k] = e2[0];       // the lower half's: entry k
                    cg.e[KH + k] = e2[1];  // the upper half's: entry KH + k
                }
                pg.load(p.gpsym + col, npad, lds_addr(L.Pv), Xbase);
            } else if (col >= 0) {
                cg.load(p.gcol + col, npad, abase, wbase);
                pg.load(p.gpsym + col, npad, lds_addr(L.Pv), Xbase);
            } else {
                cg.clear(abase + 8u * nnzA, wbase);
                pg.clear(lds_addr(L.Pv) + 8u * nnzP, Xbase);
            }
            const int oz = opaque_zero();
            double Dv, Ev;
            if constexpr (G1) {  // (E and D on chip: the one-shot form 2, edl_E / edl_D)
                Dv = col >= 0 ? edl_D(p, C)[col] : 1.0;
                Ev = ri < m ? edl_E(p, C)[ri] : 1.0;
            } else {
                Dv = col >= 0 ? opaque_gptr(p.D + b * npad)[col] : 1.0;
                Ev = ri < m ? opaque_gptr(p.E + b * m)[ri] : 1.0;
            }
            // inline update_info + check_termination (as solve_w2_body's), one row per thread
            const bool unscale = p.scaling && !p.scaled_term;
            const unsigned ysbase = lds_addr(L.ys), dYbase = lds_addr(C.dY), dxbase = lds_addr(L.dx);
            double mx[17], sm[2] = {0.0, 0.0}, adx = 0.0;
#pragma unroll
            for (int k = 0; k < 17; ++k) mx[k] = 0.0;
            {
                const bool ok = tid < m;
                double ax = 0.0, ad = 0.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const unsigned e = rg.e[k], va = e >> 16;
                    const double a = lds_at(e & 0xFFFFu);
                    ax += a * lds_at(va - xbase + Xbase);
                    ad += a * lds_at(va - xbase + dxbase);
                }
                adx = ad;
                const double zi = Z, pr = ax - zi, ei = 1.0 / Ev;
                const double lo = L.lo[ri], up = L.up[ri];
                double d = dy;
                if (up > OSQP_INFTY * MIN_SCALING) d = (lo < -OSQP_INFTY * MIN_SCALING) ? 0.0 : cmin(d, 0.0);
                else if (lo < -OSQP_INFTY * MIN_SCALING) d = cmax(d, 0.0);
                if (ok) {
                    mx[0] = fabs(ei * pr);
                    mx[2] = fabs(ei * zi);
                    mx[3] = fabs(ei * ax);
                    mx[7] = fabs(pr);
                    mx[9] = fabs(zi);
                    mx[10] = fabs(ax);
                    mx[14] = fabs(unscale ? Ev * d : d);
                    sm[0] = up * cmax(d, 0.0) + lo * cmin(d, 0.0);
                    C.dY[ri] = d;
                }
            }
            {  // the lane's column (lower half): P x, A' y, P dx, and the delta x norm
                double px = 0.0, pdx = 0.0, aty = 0.0;
#pragma unroll
                for (int k = 0; k < KPK; ++k) {
                    const unsigned e = pg.e[k], va = e >> 16;
                    const double pv = lds_at(e & 0xFFFFu);
                    px += pv * lds_at(va);
                    pdx += pv * lds_at(va - Xbase + dxbase);
                }
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const unsigned e = cg.e[k];
                    aty += lds_at(e & 0xFFFFu) * lds_at((e >> 16) - wbase + ysbase);
                }
                if (cv) {
                    const double d = (Q + px) + aty, di = 1.0 / Dv;
                    mx[1] = fabs(di * d);
                    mx[4] = fabs(di * Q);
                    mx[5] = fabs(di * aty);
                    mx[6] = fabs(di * px);
                    mx[8] = fabs(d);
                    mx[11] = fabs(Q);
                    mx[12] = fabs(aty);
                    mx[13] = fabs(px);
                    mx[15] = fabs(unscale ? Dv * DX : DX);
                    mx[16] = fabs(unscale ? pdx * di : pdx);
                }
            }
            if constexpr (ROLES) {
                if (padme) sm[1] = L.qv[tid + oz] * L.dx[tid + oz];
            } else {
            if (tid < npad && opaque_gptr(p.pad_var)[tid] >= 0) sm[1] = L.qv[tid + oz] * L.dx[tid + oz];
            }
            PH(6)  // (a check up to its reduction: write-back, operands, gathers)
            if (do_rho || !unscale) {
                block_max_sum_tr<T4, 17, 2, LEAN>(mx, sm, L.red);
            } else {
                // a check that adapts no rho decides with the unscaled norms and the
                // certificates' only: 10 maxima instead of 17 (R's scaled norms are then stale
                // and unread: only a rho step restores them)
                double m10[10] = {mx[0], mx[1], mx[2], mx[3], mx[4], mx[5], mx[6], mx[14], mx[15], mx[16]};
                block_max_sum_tr<T4, 10, 2, LEAN>(m10, sm, L.red);
#pragma unroll
                for (int k = 0; k < 7; ++k) mx[k] = m10[k];
                mx[14] = m10[7];
                mx[15] = m10[8];
                mx[16] = m10[9];
            }
            PH(7)  // (the reduction)
            Res R;
            if (unscale) {
                R.pri = mx[0]; R.dua = cscal(1) * mx[1];
                R.nz = mx[2]; R.nax = mx[3]; R.nq = mx[4]; R.naty = mx[5]; R.npx = mx[6];
            } else {
                R.pri = mx[7]; R.dua = mx[8];
                R.nz = mx[9]; R.nax = mx[10]; R.nq = mx[11]; R.naty = mx[12]; R.npx = mx[13];
            }
            R.rpri = mx[7]; R.rdua = mx[8]; R.rz = mx[9]; R.rax = mx[10]; R.rq = mx[11]; R.raty = mx[12]; R.rpx = mx[13];
            if (m == 0) R.pri = 0.0;
            if (tid == 0) R.save(L.res);
            if constexpr (LEAN) Rk = R;
            if (can_check) {
                int st = MPCQP_UNSOLVED_;
                bool done = false;
                if (R.pri > OSQP_INFTY || R.dua > OSQP_INFTY) {
                    st = MPCQP_NON_CVX_;
                    done = true;
                } else {
                    const bool prim_ok = m == 0 || R.pri < p.eps_abs + p.eps_rel * cmax(R.nz, R.nax);
                    double mxd = cmax(cmax(R.nq, R.naty), R.npx);
                    if (unscale) mxd *= cscal(1);
                    const bool dual_ok = R.dua < p.eps_abs + p.eps_rel * mxd;
                    bool prim_inf = false, dual_inf = false;
                    if (!prim_ok || !dual_ok) {
                        const double norm_dy = mx[14], norm_dx = mx[15], epi = p.eps_pinf, edi = p.eps_dinf;
                        const double cs = unscale ? cscal(0) : 1.0;
                        if (!prim_ok && m != 0 && norm_dy > epi && sm[0] < epi * norm_dy) {
                            __syncthreads();
                            double na[1] = {0.0};
                            double a = 0.0;
#pragma unroll
                            for (int k = 0; k < KC; ++k) {
                                const unsigned e = cg.e[k];
                                a += lds_at(e & 0xFFFFu) * lds_at((e >> 16) - wbase + dYbase);
                            }
                            if (cv) na[0] = fabs(unscale ? a * (1.0 / Dv) : a);
                            block_max<T4, 1>(na, L.red);
                            prim_inf = na[0] < epi * norm_dy;
                        }
                        if (!dual_ok && norm_dx > edi && sm[1] < cs * edi * norm_dx && mx[16] < cs * edi * norm_dx) {
                            bool viol = false;
                            if (tid < m) {
                                const double ar = unscale ? adx * (1.0 / Ev) : adx;
                                const double lo = L.lo[ri], up = L.up[ri];
                                if ((up < OSQP_INFTY * MIN_SCALING && ar > edi * norm_dx) ||
                                    (lo > -OSQP_INFTY * MIN_SCALING && ar < -edi * norm_dx))
                                    viol = true;
                            }
                            dual_inf = !block_any<T4>(viol, L.flag);
                        }
                    }
                    if (prim_ok && dual_ok) {
                        st = MPCQP_SOLVED_;
                        done = true;
                    } else if (prim_inf) {
                        st = MPCQP_PRIMAL_INFEASIBLE_;
                        if (tid == 0) L.flag[3] = unscale;
                        done = true;
                    } else if (dual_inf) {
                        st = MPCQP_DUAL_INFEASIBLE_;
                        if (tid == 0) L.flag[2] = unscale;
                        done = true;
                    }
                }
                // (LEAN: nothing reads the flag before the pass-end barrier, and the rho step takes
                // the residuals from Rk, not from thread 0's res)
                if constexpr (!LEAN) __syncthreads();
                // (the objective of an infeasible / non-convex status is set by finalize_ph)
                if (done && tid == 0) L.flag[1] = st;
                if constexpr (!LEAN) __syncthreads();
                status = done ? st : MPCQP_UNSOLVED_;
                stop = done;
            }
        }
        if (!stop && do_rho) {
            Res R;
            if constexpr (LEAN) {
                R = Rk;  // (every thread formed the same Res from the reduced maxima)
            } else {
                // (without a check at this iteration nothing else orders thread 0's save before this read)
                if (!can_check) __syncthreads();
                R.restore(L.res);
            }
            adapt_rho(p, R, rho, rho_updates, need_factor);
        }
        __syncthreads();
        PH(4)
        if (stop || iter >= p.max_iter) break;
    }
    const double cval = cscal(0), cinv = cscal(1);
    conclude<T4, ONE, G1>(p, b, xo, yo, cval, cinv, rho, status, can_check, iter, info_iter, rho_updates);
#ifdef MPCQP_PHASE_PROF
    if (prof) {
        __syncthreads();
        PH(5)
        if (tid == 0) {
            prof_flush(p, b, L, t0c, t0w, 14);
            p.prof[b * kProfSlots + 2] = L.pacc[12] + L.pacc[13] + L.pacc[14];
            // the check's and the tail's splits: slots 16-18 (a check up to its reduction, the
            // reduction, the run starts); 4 and 5 keep their totals
            p.prof[b * kProfSlots + 4] = L.pacc[4] + L.pacc[6] + L.pacc[7];
            p.prof[b * kProfSlots + 5] = L.pacc[5] + L.pacc[15];
            p.prof[b * kProfSlots + 16] = L.pacc[6];
            p.prof[b * kProfSlots + 17] = L.pacc[7];
            p.prof[b * kProfSlots + 18] = L.pacc[15];
        }
    }
#endif
}

// FO: the factor-only instantiation (api.hip::check_convex), so that the solve's own code
// carries no factor_only test
template <int K, int KPK, int QR, bool EL = false, int KC = K, bool FO = false, bool DK = false>
__global__ __launch_bounds__(T4, 2) void k_solve_w4(KParams p, double* __restrict__ xo, double* __restrict__ yo,
                                                    int /*factor_only: FO*/) {
    solve_w4_body<K, KPK, QR, EL, KC, DK, !FO && !DK>(p, xo, yo, FO ? 1 : 0);
    extern __shared__ __attribute__((aligned(16))) double sm[];
    order_epilogue<T4>(p, (int*)sm);
}

// setup (setup_r.h with 256 threads: one column and one row per thread) + solve; ONE: the
// one-shot form (solve_w4_body)
template <int K, int KPK, int QR, int SK, int SAS, bool EL = false, int KC = K, bool DK = false, bool ONE = false,
          int GL = 0>
__global__ __launch_bounds__(T4, 2) void k_setup_solve_w4(KParams p, const double* __restrict__ Px_in,
                                                          const double* __restrict__ Ax_in,
                                                          const double* __restrict__ q_in,
                                                          const double* __restrict__ l_in,
                                                          const double* __restrict__ u_in, double* __restrict__ xo,
                                                          double* __restrict__ yo) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    setup_r_body<T4, SK, 4, 1, SAS, 1, false, ONE, GL == 1 || GL >= 3>(p, instance_of(p), Px_in, Ax_in, q_in, l_in, u_in, sm);
    __syncthreads();
    solve_w4_body<K, KPK, QR, EL, KC, DK, false, ONE, GL>(p, xo, yo);
    order_epilogue<T4>(p, (int*)sm);
}


// Host-side guard tying an instantiation's compile-time list lengths to the plan: gather
// lists are kGS deep in memory (plan.cpp), so a shorter K never reads out of the list, but
// it would drop A entries; K / KC: row / column gather lengths, KPK: P terms per column,
// QR: nonzero G rows, K1: the slot-1 rows' length (two-wave kernel)
static hipError_t lists_fit(const KParams& p, int K, int KC, int KPK, int QR, int K1 = 1 << 30) {
    const bool ok = p.gkr <= K && p.gkc <= KC && p.gk <= std::max(K, KC) && p.pk <= KPK && p.amax <= QR &&
                    p.gk1 <= K1 && K <= kGS && KC <= kGS;
    return ok ? hipSuccess : hipErrorInvalidValue;
}

// the four-wave kernel's dense-inverse form (DK) for plans without eliminated columns whose
// blocks have at most NB0 = 26 (blocks 0, 1) / NB1 = 28 (blocks 2, 3) real columns
// (plan.cpp balances the four blocks for it): measured and not taken, so it is
// compiled into the experimental builds only, where MPCQP_DENSE_W4=1 turns it on (and the
// planner's balanced merge with it)
bool dense_w4_on() {
#ifdef MPCQP_EXPERIMENTAL
    static const bool on = [] {
        const char* e = getenv("MPCQP_DENSE_W4");
        return e && e[0] == '1';
    }();
    return on;
#else
    return false;
#endif
}
[[maybe_unused]] static bool dense_w4(const KParams& p) {
    return dense_w4_on() && p.ne == 0 && p.Kd && p.bsz01 <= 26 && p.bsz23 <= 28;
}

int one_shot_form(const KParams& p, size_t* lds) {
    const Variant* d = variant_of(p.variant);  // the fused four-wave kernel's variants only
    if (!d || d->setup_solve != launch_setup_solve_w4 || p.polish) return 0;
    const size_t base = std::max(lds_w2_bytes(p), lds_setup_r_bytes(p.nnzP, p.nnzA, p.npad, p.m));
    // (form 2: the G blocks and the y of a refactorisation, which the factorisation's E tiles
    // overwrite in the carve, after the S_k^{-1} tiles)
    const size_t g = sizeof(double) * ((size_t)(p.nb * (p.nb - 1) / 2) * p.amax * S + (size_t)p.m);
    // form 3 (GL 2): the G blocks straight into the solve's gl copy, with factorize_w4_gl's
    // scratch (the E tiles and wave buffers) in the carve's V span before gl
    // form 2 also keeps E and D after gl (edl_E / edl_D: the V span's room past gl)
    const long vspan = 3L * solve_mpad(p.m) + 2L * p.npad;
    const long vfree = solve_vlen(p.m, p.npad, p.nb, p.amax, p.mode) - vspan - solve_glen(p.nb, p.amax, p.mode);
    const bool edl = vfree >= ((p.m + 1) & ~1) + p.npad;
    const int form = base + g <= 80 * 1024 && edl ? 2 : (p.amax <= 8 && 4L * p.amax * S + 8 * S + 8 <= vspan ? 3 : 1);
    if (lds) *lds = form == 2 ? base + g : base;
    return form;
}

// The four-wave kernel's instantiations, one shape per kind of plan (solve.hip's table gives the
// preconditions): K / KC the row / column gather-list lengths, KPK the P terms per column, QR the
// rows of the G blocks phase C sums (the nonzero ones: amax), SK / SAS the fused setup's list
// length and A values per thread, EL eliminated columns (the slack layouts)
template <int K_, int KPK_, int QR_, int SK_, int SAS_, bool EL_, int KC_>
struct W4Shape {
    static constexpr int K = K_, KPK = KPK_, QR = QR_, SK = SK_, SAS = SAS_, KC = KC_;
    static constexpr bool EL = EL_;
    template <bool FO = false, bool DK = false>
    static constexpr auto solve() { return k_solve_w4<K, KPK, QR, EL, KC, FO, DK>; }
    template <bool ONE = false, int GL = 0, bool DK = false>
    static constexpr auto setup_solve() { return k_setup_solve_w4<K, KPK, QR, SK, SAS, EL, KC, DK, ONE, GL>; }
    // the plan's lists fit the instantiation's (a shorter list would silently drop A entries)
    static hipError_t fits(const KParams& p) { return lists_fit(p, K, KC, KPK, QR); }
};
using W4Elim = W4Shape<6, 4, 8, 8, 3, true, 8>;    // eliminated columns
using W4Five = W4Shape<6, 4, 5, 6, 2, false, 6>;   // amax <= 5 (cfg 2, the headline)
using W4Rest = W4Shape<6, 4, 8, 6, 2, false, 6>;
// f(shape) for the plan's shape
template <class F>
static auto with_w4_shape(const KParams& p, F f) {
    if (p.ne) return f(W4Elim{});
    if (p.amax <= 5) return f(W4Five{});
    return f(W4Rest{});
}

// the one-shot fused kernel's GL (solve_w4_body) for one_shot_form `form` > 0
constexpr int one_shot_gl(int form, bool el, bool qr5, bool ab5, OneShot loop) {
    if (form != 2) return form == 3 ? 2 : 0;
    if (el || !qr5) return 1;
    const int best = ab5 ? 5 : 4;
    const int cap = loop == OneShot::lds ? 1 : loop == OneShot::wave ? 3 : loop == OneShot::roles ? 4 : 5;
    return cap < best ? cap : best;
}
static_assert(one_shot_gl(2, false, true, true, OneShot::dflt) == 5 && one_shot_gl(2, false, true, false, OneShot::dflt) == 4);
static_assert(one_shot_gl(2, false, true, true, OneShot::roles) == 4 && one_shot_gl(2, false, true, false, OneShot::roles) == 4);
static_assert(one_shot_gl(2, false, true, true, OneShot::wave) == 3 && one_shot_gl(2, false, true, false, OneShot::wave) == 3);
static_assert(one_shot_gl(2, false, true, true, OneShot::lds) == 1 && one_shot_gl(2, false, true, false, OneShot::lds) == 1);
static_assert(one_shot_gl(1, false, true, true, OneShot::dflt) == 0 && one_shot_gl(3, false, true, true, OneShot::dflt) == 2);
static_assert(one_shot_gl(2, true, false, true, OneShot::dflt) == 1 && one_shot_gl(2, false, false, true, OneShot::dflt) == 1);

int one_shot_kernel(const KParams& p, OneShot loop, size_t* lds) {
    const int form = loop == OneShot::off ? 0 : one_shot_form(p, lds);
    return form ? one_shot_gl(form, p.ne != 0, p.amax <= 5, p.amax == 5 && p.bmax == 5, loop) : -1;
}

// the four-wave kernel's fused launch (variant_fits covers its preconditions: list lengths,
// pk <= 4, nnzA <= 2 or 3 x T4); one-shot: the instantiation one_shot_kernel names
hipError_t launch_setup_solve_w4(const KParams& p, long B, const double* Px, const double* Ax, const double* q,
                                 const double* l, const double* u, double* xo, double* yo, hipStream_t st,
                                 OneShot one_shot) {
    size_t lds = 0;
    const int gl = one_shot_kernel(p, one_shot, &lds);
    if (gl < 0) lds = std::max(lds_w2_bytes(p), lds_setup_r_bytes(p.nnzP, p.nnzA, p.npad, p.m));
    using Kernel = decltype(W4Five::setup_solve());
    const Kernel k4 = with_w4_shape(p, [&](auto sh) -> Kernel {
        using Sh = decltype(sh);
        constexpr bool five = !Sh::EL && Sh::QR <= 5;  // (one_shot_gl gives 3, 4, 5 on this shape only)
        switch (gl) {  // (the cases' order is the kernels' order in the code object: tools/codeobj.py's hash)
            case 3: if constexpr (five) return Sh::template setup_solve<true, 3>(); break;
            case 5: if constexpr (five) return Sh::template setup_solve<true, 5>(); break;
            case 4: if constexpr (five) return Sh::template setup_solve<true, 4>(); break;
            case 1: return Sh::template setup_solve<true, 1>();
            case 2: return Sh::template setup_solve<true, 2>();
            case 0: return Sh::template setup_solve<true>();
        }
#ifdef MPCQP_EXPERIMENTAL
        if constexpr (five)
            if (dense_w4(p)) return Sh::template setup_solve<false, 0, true>();
#endif
        return Sh::setup_solve();
    });
    hipError_t e = with_w4_shape(p, [&](auto sh) { return decltype(sh)::fits(p); });
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)k4, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k4, dim3((unsigned)B), dim3(T4), lds, st, p, Px, Ax, q, l, u, xo, yo);
    e = hipGetLastError();
    if (e != hipSuccess || !p.polish) return e;  // (a one-shot form implies no polish: one_shot_form)
    return launch_polish(p, B, xo, yo, st);
}

// the two-wave kernel's fused launch where the 128-thread register-list setup shape holds (one
// padded column per thread, two rows, four A values), else the two kernels
hipError_t launch_setup_solve_w2(const KParams& p, long B, const double* Px, const double* Ax, const double* q,
                                 const double* l, const double* u, double* xo, double* yo, hipStream_t st,
                                 OneShot /*one_shot*/) {
    if (!(p.npad <= T2 && p.m <= 2 * T2 && p.gk <= 6 && p.pk <= 4 && p.nnzA <= 4 * T2 && p.nnzP <= 2 * T2)) {
        hipError_t e = launch_setup(p, B, Px, Ax, q, l, u, st);
        return e != hipSuccess ? e : launch_solve(p, B, xo, yo, 0, st);
    }
    const size_t lds = std::max(lds_w2_bytes(p), lds_setup_r_bytes(p.nnzP, p.nnzA, p.npad, p.m));
    auto k = p.gk1 <= 1 ? k_setup_solve_w2<6, 2, 4, 1, 6, 2, 4, 2> : k_setup_solve_w2<6, 2, 4, 6, 6, 2, 4, 2>;
    hipError_t e = lists_fit(p, 6, 6, 4, 1 << 30, 6);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(T2), lds, st, p, Px, Ax, q, l, u, xo, yo);
    e = hipGetLastError();
    if (e != hipSuccess || !p.polish) return e;
    return launch_polish(p, B, xo, yo, st);
}

template <int K, int RS, int KPK, int K1>
static hipError_t go_w2(const KParams& p, long B, double* xo, double* yo, int fo, hipStream_t st, size_t lds,
                        KernelRef* ref) {
    auto k = k_solve_w2<K, RS, KPK, K1>;
    hipError_t e = lists_fit(p, K, K, KPK, 1 << 30, K1);
    if (e != hipSuccess) return e;
    if (ref) { *ref = {(const void*)k, T2, lds}; return hipSuccess; }
    e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(T2), lds, st, p, xo, yo, fo);
    return hipGetLastError();
}

// the two-wave kernel's LDS: the carve plus the nb S_k^{-1} tiles
size_t lds_w2_bytes(const KParams& p) {
    return 16 * ((lds_base_bytes(p) + 15) / 16) + sizeof(double) * (size_t)p.nb * SS;
}

// the four-wave kernel's solve (FO: setup()'s convexity check)
hipError_t launch_solve_w4(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                           KernelRef* ref) {
    using Kernel = decltype(W4Five::solve());
    const Kernel k = with_w4_shape(p, [&](auto sh) -> Kernel {
        using Sh = decltype(sh);
        if (factor_only) return Sh::template solve<true>();
#ifdef MPCQP_EXPERIMENTAL
        if constexpr (!Sh::EL && Sh::QR <= 5)
            if (dense_w4(p)) return Sh::template solve<false, true>();
#endif
        return Sh::solve();
    });
    const size_t lds = lds_w2_bytes(p);
    hipError_t e = with_w4_shape(p, [&](auto sh) { return decltype(sh)::fits(p); });
    if (e != hipSuccess) return e;
    if (ref) { *ref = {(const void*)k, T4, lds}; return hipSuccess; }
    e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((unsigned)B), dim3(T4), lds, st, p, xo, yo, factor_only);
    return hipGetLastError();
}

// The two-wave kernel's: slot-1 rows (>= 128) with at most one nonzero (cfg 2's box rows): K1 = 1
hipError_t launch_solve_w2(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                           KernelRef* ref) {
    return p.gk1 <= 1 ? go_w2<6, 2, 4, 1>(p, B, xo, yo, factor_only, st, lds_w2_bytes(p), ref)
                      : go_w2<6, 2, 4, 6>(p, B, xo, yo, factor_only, st, lds_w2_bytes(p), ref);
}

}  // namespace mpcqp
