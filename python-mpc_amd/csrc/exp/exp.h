// exp.h -- the kernels measured and not taken: what their translation
// units in this directory declare to variants.hip, which registers them with solve.hip's
// table in the experimental builds (MPCQP_EXPERIMENTAL: libmpcqp_exp.so, the prof / skew builds).
#pragma once
#include "../kernels.h"

namespace mpcqp {

constexpr int kDenseR = 104;  // solve_dense.hip: register row length of M^{-1} (variables per QP)

// one-wave-per-QP kernel (solve_wave1.hip), variants 8 and 9
hipError_t launch_solve_wave1(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                              KernelRef* ref = nullptr);
// eight-wave kernel (solve_wave8.hip), variant 18
hipError_t launch_solve_wave8(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                              KernelRef* ref = nullptr);
// dense-inverse kernel (solve_dense.hip), variant 16, and its LDS bytes
hipError_t launch_solve_dense(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                              KernelRef* ref = nullptr);
size_t lds_dense_bytes(const KParams& p);
// one 512-thread workgroup per QP, alone on its CU, the dense-inverse solve held in registers
// (solve_heavy.hip, variant 19): the latency form for a batch's predicted-slowest instances
bool heavy_fits(const KParams& p);
size_t heavy_lds(const KParams& p);
hipError_t launch_solve_heavy(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                              KernelRef* ref = nullptr);
hipError_t launch_setup_solve_heavy(const KParams& p, long B, const double* Px, const double* Ax, const double* q,
                                    const double* l, const double* u, double* xo, double* yo, hipStream_t st);
// the long-horizon kernel's 256-thread and two-wave instantiations (../solve_big.hip), variants 15 and 14
hipError_t launch_solve_big18_256(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                                  KernelRef* ref = nullptr);
hipError_t launch_solve_big8_w2(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                                KernelRef* ref = nullptr);

}  // namespace mpcqp
