// mpc_assembly.hip -- the MPC data path around the solver, on the device:
// the QP layouts and the assembly of their values from the linearised stages, batched over B
// vehicles, with the assembly's transposes.
//
//   F1  k_incr_assemble_A / _vec      mpc_increment's QP values            mpc_dynamics.py:281-389
// and the LTV MPC in the inputs themselves (mpcqp_ltv_layout: the same layout with nxa = nx, the
// same two assembly kernels), and for the one closed loop that keeps its problem alive,
// vehicle_lateral_mpc_slack_increment.py (setup once, update(q, l, u) + warm-started solve per
// step), k_affine assembles its vectors.
//
// One thread per vehicle for the vectors; one thread per (vehicle, A entry) for the assembly,
// which is a scatter of stage blocks into the shared CSC pattern.  All fp64.  No kernel here takes
// a vehicle.
//
// Each host function below is followed by the entry points that forward to it, incr_ then ltv_.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/mpcqp.h"
#include "kernels.h"
#include "mpc_host.h"
#include "mpc_layout.h"

namespace mpcqp {

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

}  // namespace mpcqp

using namespace mpcqp;

struct mpcqp_affine {
    int dev = 0, L = 0, R = 0, T = 0, seg0 = 0, seg1 = 0, nparam = 0;
    double *d_base = nullptr, *d_coef = nullptr;
    int* d_idx = nullptr;
    // the terms by parameter (for the VJP): parameter p's are pent / pcoef[pptr[p] .. pptr[p+1])
    int *d_pptr = nullptr, *d_pent = nullptr;
    double* d_pcoef = nullptr;
};

// P = blockdiag(kron(I_N, C'QC), C'QN C, kron(I_N, R)), upper triangle, zeros dropped
// (mpc_dynamics.py:304-307); with nxa = nx, C = I: blockdiag(Q x N, QN, R x N)
static void build_P(IncrLayout& L, const double* Q, const double* QN, const double* R) {
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

// P, the A pattern with its source codes, and Qt of a layout with nxa >= nx state columns per
// stage (:336-369, :381-382; mpc_kinematics_pred_matrix.py:293-309, :326, :341 for nxa = nx).
// The bounds (set_box) are the caller's.
static void build_layout(IncrLayout& L, int N, int nx, int nu, int nxa, int device, const double* Q, const double* QN,
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

extern "C" {
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
}  // extern "C"

// dims / pattern / free of either layout (mpcqp_incr_layout, mpcqp_ltv_layout)
static int layout_dims(const IncrLayout* L, const char* what, int32_t* n, int32_t* m, int32_t* nnzP, int32_t* nnzA) {
    if (!L || !n || !m || !nnzP || !nnzA) return set_error(MPCQP_EINVAL, "%s: NULL argument", what);
    *n = L->n; *m = L->m; *nnzP = (int32_t)L->Pi.size(); *nnzA = (int32_t)L->Ai.size();
    return 0;
}

extern "C" {
int mpcqp_incr_layout_dims(const mpcqp_incr_layout* L, int32_t* n, int32_t* m, int32_t* nnzP, int32_t* nnzA) {
    return layout_dims(L, "incr_layout_dims", n, m, nnzP, nnzA);
}

int mpcqp_ltv_layout_dims(const mpcqp_ltv_layout* L, int32_t* n, int32_t* m, int32_t* nnzP, int32_t* nnzA) {
    return layout_dims(L, "ltv_layout_dims", n, m, nnzP, nnzA);
}
}  // extern "C"

static int layout_pattern(const IncrLayout* L, const char* what, int32_t* Pp, int32_t* Pi, double* Px, int32_t* Ap,
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

extern "C" {
int mpcqp_incr_layout_pattern(const mpcqp_incr_layout* L, int32_t* Pp, int32_t* Pi, double* Px, int32_t* Ap,
                              int32_t* Ai, double* Ax_template, double* l_template, double* u_template) {
    return layout_pattern(L, "incr_layout_pattern", Pp, Pi, Px, Ap, Ai, Ax_template, l_template, u_template);
}

int mpcqp_ltv_layout_pattern(const mpcqp_ltv_layout* L, int32_t* Pp, int32_t* Pi, double* Px, int32_t* Ap,
                             int32_t* Ai, double* Ax_template, double* l_template, double* u_template) {
    return layout_pattern(L, "ltv_layout_pattern", Pp, Pi, Px, Ap, Ai, Ax_template, l_template, u_template);
}
}  // extern "C"

static void layout_free_device(IncrLayout* L) {
    if (L->d_asrc) (void)hipSetDevice(L->dev);
    if (!L->d_asrc && L->d_Qtw) (void)hipSetDevice(L->dev);
    for (void* p : {(void*)L->d_asrc, (void*)L->d_Atpl, (void*)L->d_ltpl, (void*)L->d_utpl, (void*)L->d_Qt,
                    (void*)L->d_adst, (void*)L->d_bdst, (void*)L->d_psrc, (void*)L->d_wptr, (void*)L->d_wlist,
                    (void*)L->d_W, (void*)L->d_Qtw})
        if (p) (void)hipFree(p);
}

extern "C" {
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
}  // extern "C"

// dxlo, dxhi: per-stage state bounds (B, N+1, nxa), either may be null
static int assemble_device(const char* what, const IncrLayout* L, int64_t B, const double* dAd, const double* dBd,
                           const double* dgd, const double* dx0, const double* dXr, const double* dxlo,
                           const double* dxhi, double* dAx, double* dq, double* dl, double* du, void* stream) {
    if (!L || !dAd || !dBd || !dgd || !dx0 || !dXr || !dAx || !dq || !dl || !du || B < 0)
        return set_error(MPCQP_EINVAL, "%s: bad arguments", what);
    if (B == 0) return 0;
    if (int e = ensure_device(*const_cast<IncrLayout*>(L))) return e;
    const IncrK k = incr_k(*L);
    if (int e = launch(L->dev, stream, B * k.nnzA, 256, k_incr_assemble_A, k, B, dAd, dBd, dAx)) return e;
    return launch(L->dev, stream, B, 128, k_incr_assemble_vec, k, B, dgd, dx0, dXr, dxlo, dxhi, dq, dl, du);
}

extern "C" {
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
}  // extern "C"

// assemble_device with the weights of this call (each null: the layout's own): k_weights writes
// the Qt scratch and dPx, then the forward kernels run unchanged with IncrK::Qt on the scratch
static int assemble_w_device(const char* what, const IncrLayout* L, int64_t B, const double* dAd, const double* dBd,
                             const double* dgd, const double* dx0, const double* dXr, const double* dxlo,
                             const double* dxhi, const double* dQ, const double* dQN, const double* dR, double* dAx,
                             double* dq, double* dl, double* du, double* dPx, void* stream) {
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

extern "C" {
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
}  // extern "C"

// The transpose of assemble_device (and of assemble_w_device: dQ / dQN the weights that call took,
// null the layout's own).  Every cotangent and every output may be null.
static int assemble_vjp_device(const char* what, const IncrLayout* L, int64_t B, const double* dgPx,
                               const double* dgAx, const double* dgq, const double* dgl, const double* dgu,
                               const double* dXr, const double* dxlo, const double* dxhi, const double* dQ,
                               const double* dQN, double* dgAd, double* dgBd, double* dggd, double* dgx0, double* dgXr,
                               double* dgxlo, double* dgxhi, double* dgQ, double* dgQN, double* dgR, void* stream) {
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

extern "C" {
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
}  // extern "C"

// ---- the affine vector assembly (k_affine) ----

extern "C" {
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
}  // extern "C"
