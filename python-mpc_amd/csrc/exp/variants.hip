// variants.hip -- the descriptors (kernels.h, struct Variant) of the variants measured and not
// taken: one-wave 8 / 9, two-wave two-sided 14, 256-thread twisted 15, dense inverse 16,
// eight-wave 18, one-instance-per-CU dense 19.  solve.hip's table takes them in the
// experimental builds; none is in solve_variant's preference order (MPCQP_VARIANT only).
#include "../solve_phases.h"
#include "exp.h"

namespace mpcqp {

// the one-wave kernels' rows i = lane + 64 s, s < RS, must cover exactly the padded rows
// (solve_mpad): RS = 3 for 128 < m <= 192, RS = 4 for 192 < m <= 256
static bool fits8(const KParams& p) {
    return p.nb == 4 && p.amax <= 8 && p.gk <= 6 && solve_mpad(p.m) == 3 * 64 && lds_solve_bytes(p) < 65536;
}
static bool fits9(const KParams& p) {
    return p.nb == 4 && p.amax <= 8 && p.gk <= 8 && solve_mpad(p.m) == 4 * 64 && lds_solve_bytes(p) < 65536;
}
static bool fits14(const KParams& p) {
    return p.nb > 4 && p.nb <= 8 && p.amax <= 16 && p.bmax <= 16 && p.gk <= 8 && p.npad <= 256 &&
           p.m <= 256 && lds_solve_bytes_big(p) <= 160 * 1024;
}
static bool fits15(const KParams& p) {  // 256 threads, one wave per SIMD (twisted_solve4): nb <= 18
    const int csb = (p.npad + 255) / 256, rsb = (p.m + 255) / 256;
    return p.nb > 4 && p.nb <= 18 && p.amax <= 16 && p.bmax <= 16 && p.gk <= 8 && csb <= 3 && rsb <= 4 &&
           lds_solve_bytes_big(p) <= 160 * 1024;
}
// dense inverse: one variable per lane pair of a 256-thread workgroup, packed LDS addresses
static bool fits16(const KParams& p) {
    return p.n <= kDenseR && p.npad <= 128 && p.gk <= 6 && p.pk <= 4 && p.m <= 2 * 128 &&
           lds_dense_bytes(p) < 65536;
}
static bool fits18(const KParams& p) {  // eight waves, one workgroup per CU; the gather lists pack 16-bit LDS addresses
    KParams q2 = p;
    q2.mode = 2;  // the LDS carve of mode 2 (fits may run before KParams::mode is set)
    const long mp = solve_mpad(p.m), packed = 8L * (al2(p.nnzA + 1) + al2(p.nnzP + 1) + 4 * mp + 4L * p.npad);
    return p.nb == 8 && p.amax <= 12 && p.gk <= 8 && p.pk <= 8 && p.m <= 512 && p.npad <= 256 &&
           packed < 65536 && lds_solve_bytes(q2) <= 160 * 1024;
}

static hipError_t launch19(const KParams& p, long B, double* xo, double* yo, int factor_only, hipStream_t st,
                           KernelRef* ref) {
    if (!factor_only) return launch_solve_heavy(p, B, xo, yo, 0, st, ref);
    KParams q = p;  // setup()'s convexity factorisation: the four-wave kernel's (the same factor)
    q.variant = 17;
    return launch_solve_w4(q, B, xo, yo, factor_only, st, ref);
}
static hipError_t setup_solve19(const KParams& p, long B, const double* Px, const double* Ax, const double* q,
                                const double* l, const double* u, double* xo, double* yo, hipStream_t st,
                                OneShot /*one_shot*/) {
    hipError_t e = launch_setup_solve_heavy(p, B, Px, Ax, q, l, u, xo, yo, st);
    return (e != hipSuccess || !p.polish) ? e : launch_polish(p, B, xo, yo, st);
}

// id, threads, mode, order, elim, fits, lds, launch, setup_solve
static const Variant kExpVariants[] = {
    {8, 64, 2, false, false, fits8, lds_solve_bytes, launch_solve_wave1, nullptr},
    {9, 64, 2, false, false, fits9, lds_solve_bytes, launch_solve_wave1, nullptr},
    {14, 128, 3, false, false, fits14, lds_solve_bytes_big, launch_solve_big8_w2, nullptr},
    {15, 256, 3, false, false, fits15, lds_solve_bytes_big, launch_solve_big18_256, nullptr},
    {16, 256, 1, false, false, fits16, lds_dense_bytes, launch_solve_dense, nullptr},  // (no factor stored; dx aliases rb)
    {18, 512, 2, false, false, fits18, lds_solve_bytes, launch_solve_wave8, nullptr},
    {19, 512, 2, true, false, heavy_fits, heavy_lds, launch19, setup_solve19},
};

int exp_variants(const Variant** list) {
    *list = kExpVariants;
    return (int)(sizeof(kExpVariants) / sizeof(kExpVariants[0]));
}

}  // namespace mpcqp
