// mpc_layout.h -- the QP layout objects of the MPC data path as the files that use one see them:
// mpc_assembly.hip builds a layout and defines the functions declared here, mpc_device.hip's loop
// tails read its sizes and device arrays through them.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/mpcqp.h"

namespace mpcqp {

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

// mpc_assembly.hip: the layout's device arrays, uploaded by the first call that needs them
// (ensure_reverse: the reverse maps, the caller's weights and the per-call Qt scratch), and the
// by-value view of an uploaded layout
int ensure_device(IncrLayout& L);
int ensure_reverse(IncrLayout& L);
IncrK incr_k(const IncrLayout& L);

}  // namespace mpcqp

struct mpcqp_incr_layout : mpcqp::IncrLayout {};
struct mpcqp_ltv_layout : mpcqp::IncrLayout {};  // nxa = nx: no augmentation
