/*
 * mpcqp.h -- C ABI of the MI355X batched linear-MPC QP solver (libmpcqp.so).
 *
 * Drop-in boundary for the reference's `osqp.OSQP()` call sites.  Each entry
 * point below replaces one step of the reference's OSQP usage:
 *
 *   mpcqp_setup_batch     <- prob = osqp.OSQP(); prob.setup(P, q, A, l, u, **settings)
 *                            vehicle_lateral_mpc_slack_increment.py:118,121
 *                            Control/MPC/mpc_kinematics.py:194-195
 *                            Control/MPC/mpc_dynamics.py:240-241,392-393
 *                            Control/MPC/mpc_kinematics_pred_matrix.py:195-196,260-261,346-347
 *                            Control/MPC/mpc_increment_kinematics_pred_matrix.py:241-242
 *                            Control/MPC/mpc_bottleneck_check.py:197-198
 *                            Control/MPC/mpc_incre_kine_func.py:179-180
 *   mpcqp_update_batch    <- prob.update(q=q_new, l=l_new, u=u_new)
 *                            vehicle_lateral_mpc_slack_increment.py:237,269
 *   mpcqp_update_settings <- prob.update_settings(**kwargs)   (osqp API; not called by the reference)
 *   mpcqp_update_matrices_batch <- prob.update(Px=, Px_idx=, Ax=, Ax_idx=)
 *                            vehicle_lateral_mpc_slack_increment.py:236 (commented out there)
 *   mpcqp_warm_start_batch<- prob.warm_start(x=..., y=...)   (osqp API; used for
 *                            the receding-horizon shift)
 *   mpcqp_solve_batch     <- res = prob.solve(); res.x, res.y, res.info.status, res.info.iter
 *                            vehicle_lateral_mpc_slack_increment.py:248,252,256
 *                            Control/MPC/mpc_dynamics.py:396,406-407
 *   mpcqp_free            <- end of the OSQP object's lifetime
 *
 * One handle holds B independent QP instances that SHARE one sparsity pattern
 * (P upper-triangular CSC n x n, A CSC m x n, int32, 0-based) and carry their
 * own values.  Per-instance arrays are instance-major:  Px[B*nnzP], Ax[B*nnzA],
 * q[B*n], l[B*m], u[B*m], x[B*n], y[B*m].  Values follow the order of the
 * pattern's data arrays (osqp-python keeps triu(P) in CSC order).
 *
 * Ownership: every input is copied into device memory during the call; the
 * caller may free or reuse its buffers afterwards.  Outputs go to
 * caller-allocated buffers.  Host-pointer entry points block until results
 * are on the host; *_device entry points take device pointers on the
 * handle's (single) device and enqueue on `stream` (hipStream_t, NULL = the
 * handle's own stream) without synchronising.  Calls on one handle are
 * stream-ordered by the library: they share the handle's workspace, including
 * the dispatch order each solve rewrites for the next one (longest previous
 * solve first; setting MPCQP_DISPATCH=identity before mpcqp_create /
 * mpcqp_setup_batch turns it off), so a call enqueued on a different stream
 * than the previous call on the handle first waits (hipStreamWaitEvent) for
 * that call's work.  The caller still orders its own buffers (inputs written
 * on another stream, outputs read elsewhere).  The order moves instances
 * between workgroups, never their results.
 *
 * Errors: entry points return 0 on success or an MPCQP_E* code; the message
 * is in mpcqp_last_error() (thread-local).  Numerical outcomes never fail a
 * call: they are reported per instance in status[] with OSQP's values.
 * A handle must be used from one host thread at a time.
 */
#ifndef MPCQP_H
#define MPCQP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* per-instance status (same values as OSQP's constants.h) */
#define MPCQP_DUAL_INFEASIBLE_INACCURATE 4
#define MPCQP_PRIMAL_INFEASIBLE_INACCURATE 3
#define MPCQP_SOLVED_INACCURATE 2
#define MPCQP_SOLVED 1
#define MPCQP_MAX_ITER_REACHED (-2)
#define MPCQP_PRIMAL_INFEASIBLE (-3)
#define MPCQP_DUAL_INFEASIBLE (-4)
#define MPCQP_NON_CVX (-7)
#define MPCQP_UNSOLVED (-10)

/* call error codes */
#define MPCQP_OK 0
#define MPCQP_EINVAL 1        /* bad argument / data validation (e.g. l > u) */
#define MPCQP_EUNSUPPORTED 2  /* sparsity structure or setting not supported */
#define MPCQP_EDEVICE 3       /* HIP runtime error / no device */
#define MPCQP_ENOMEM 4
#define MPCQP_ENONCVX 5       /* mpcqp_setup_batch: an instance's P is not convex (OSQP_NONCVX_ERROR) */

typedef struct {
    double rho, sigma, alpha;
    double eps_abs, eps_rel, eps_prim_inf, eps_dual_inf;
    double adaptive_rho_tolerance;
    int32_t max_iter, scaling, check_termination, warm_start;
    int32_t adaptive_rho, adaptive_rho_interval, scaled_termination, polish, verbose;
    double delta;                 /* polish regularisation (OSQP default 1e-6) */
    int32_t polish_refine_iter;   /* polish iterative-refinement steps (OSQP default 3) */
} mpcqp_settings;

typedef struct {
    int32_t n, m, nb, block, npad, max_level;
    int64_t batch;
    int32_t n_devices;
    int64_t lds_bytes_solve;    /* dynamic LDS per workgroup of the ADMM kernel */
    int64_t bytes_per_instance; /* device workspace per instance */
    int32_t amax;               /* coupling rows of the off-diagonal blocks */
    int32_t gather_k;           /* max nonzeros per row / column of A */
    int32_t variant;            /* solve-kernel instantiation in use */
    int32_t threads_per_qp;     /* workgroup size of that kernel */
    int32_t n_eliminated;       /* variables taken out of the block system by a scalar Schur
                                   complement (degree <= 1 vertices of K: slack columns) */
    int32_t plan_choice;        /* 0 plain plan (elimination not tried: polish, MPCQP_ELIM=0, a
                                   variant override), 1 eliminated plan, 2 an eliminated plan was
                                   built but did not fit the four-wave kernel (the reason:
                                   mpcqp_plan_preview's note; MPCQP_PLAN_LOG=1 prints it),
                                   3 nothing to eliminate */
} mpcqp_plan_info;

typedef struct mpcqp_handle mpcqp_handle;

/* OSQP 0.6 defaults; adaptive_rho_interval = 0 resolves to 4*check_termination
 * (OSQP's non-profiling rule, pinned). */
void mpcqp_default_settings(mpcqp_settings *s);

/* Symbolic analysis + allocation + per-instance setup (scaling, rho classes).
 * device_mask: bit d selects HIP device d; 0 = device 0.  The batch is split
 * into contiguous shards across the selected devices (no collectives): every
 * shard's kernels are enqueued (one stream per shard) before the host gathers
 * the results, so the devices run concurrently.  MPCQP_SPLIT=k in the
 * environment (diagnostic) cuts k shards per selected device. */
int mpcqp_setup_batch(int32_t n, int32_t m,
                      const int32_t *Pp, const int32_t *Pi,
                      const int32_t *Ap, const int32_t *Ai,
                      int64_t B, const double *Px, const double *Ax,
                      const double *q, const double *l, const double *u,
                      const mpcqp_settings *settings, uint32_t device_mask,
                      mpcqp_handle **out);

/* (mpcqp_setup_batch, as osqp_setup) returns MPCQP_ENONCVX when an instance's KKT matrix is
 * not quasi-definite (P + sigma I + A' diag(rho) A not positive definite): one factor-only
 * launch of the solve kernel checks every instance.  The device entry points do not check;
 * their solve reports such an instance as non-convex (status -7). */
/* q, l, u may each be NULL (not updated). */
int mpcqp_update_batch(mpcqp_handle *h, const double *q, const double *l, const double *u);
/* osqp_update_P / osqp_update_A / osqp_update_P_A (OSQP 0.6): new values of P's upper
 * triangle and / or A for every instance -- Px is B x nPx, Ax is B x nAx, row-major; each
 * row holds the values at the indices Px_idx / Ax_idx (into the value arrays given to
 * mpcqp_setup_batch, in its CSC order; a repeated index takes its last value), or all
 * nnzP / nnzA values when the index array is NULL (n* then ignored).  Either matrix may be
 * NULL.  As OSQP: the data is unscaled, updated, scaled afresh and refactored at the next
 * solve; x, z, y, rho and the row classes are kept (the iterates stay in the previous
 * scaling).  The sparsity pattern is fixed.  Handles of mpcqp_setup_batch only, not in
 * shared-matrix mode.  MPCQP_ENONCVX when the new matrices are not convex (OSQP's update
 * refactors at once).  Replaces prob.update(Px=, Px_idx=, Ax=, Ax_idx=), which the reference
 * mentions at vehicle_lateral_mpc_slack_increment.py:236 (commented out). */
int mpcqp_update_matrices_batch(mpcqp_handle *h, const double *Px, const int32_t *Px_idx, int32_t nPx,
                                const double *Ax, const int32_t *Ax_idx, int32_t nAx);
/* osqp_warm_start / osqp_warm_start_x / osqp_warm_start_y (OSQP 0.6): x, y may each be NULL
 * (keeps the current iterate of that part).  With x: x = D^-1 x0 and z = A x.  With y alone:
 * y = c E^-1 y0, and x and z stay as the last solve (or setup) left them -- after a solve z is
 * not A x, and OSQP keeps it too.  Turns the warm_start setting on. */
int mpcqp_warm_start_batch(mpcqp_handle *h, const double *x, const double *y);
/* osqp_update_settings / osqp_update_rho (OSQP 0.6; osqp-python's update_settings): max_iter,
 * eps_abs, eps_rel, eps_prim_inf, eps_dual_inf, rho (with set_rho != 0 only, as osqp-python
 * calls update_rho only when rho is passed: clipped to [1e-6, 1e6], every instance, refactored
 * at the next solve; else each instance keeps the rho its solves adapted to), alpha, delta, polish, polish_refine_iter, scaled_termination,
 * check_termination, warm_start take the new values; sigma, scaling and the adaptive-rho
 * settings must be unchanged (MPCQP_EINVAL otherwise), as OSQP fixes them at setup.  Any
 * handle.  polish = 1 on a handle whose plan eliminated variables (the slack layouts set up
 * without polish) moves the handle onto the plain plan first (polish factors all of K): its
 * data, scaling, iterates, rho and row classes are kept, so the next solve continues exactly
 * as on a handle set up with polish on. */
int mpcqp_update_settings(mpcqp_handle *h, const mpcqp_settings *s, int32_t set_rho);
/* any output may be NULL.  Every solve starts from the status "unsolved" and reports its own
 * conclusion.  (OSQP 0.6's osqp_solve keeps info.status_val of the previous solve when no
 * osqp_update_* call came in between -- only those reset it -- and then skips the approximate
 * check at the iteration cap: solve, warm_start, solve can report the first solve's "solved
 * inaccurate" for a second one that is not.  With an update call between two solves, as the
 * reference's loops make, the two agree.) */
int mpcqp_solve_batch(mpcqp_handle *h, double *x, double *y, int32_t *status, int32_t *iters);
/* info of the last solve; any output may be NULL */
int mpcqp_get_info_batch(mpcqp_handle *h, double *obj_val, double *pri_res, double *dua_res,
                         double *rho_estimate, int32_t *rho_updates);
/* infeasibility certificates of the last solve (OSQP res.prim_inf_cert / dua_inf_cert) */
/* res.info.status_polish per instance (osqp polish.c, run after the solve when
 * settings.polish): 0 not run (status not "solved" or polish off), 1 the polished
 * solution was taken (x, y, obj_val, pri_res, dua_res are the polished ones), -1
 * polishing did not improve the residuals (the ADMM solution stands). */
int mpcqp_get_polish_status(mpcqp_handle *h, int32_t *status_polish);
int mpcqp_get_certificates(mpcqp_handle *h, double *prim_inf_cert, double *dual_inf_cert);

/* ---- device-resident entry points (single-device handles) ---- */
/* Allocate a handle with its workspace but no data (pattern only). */
int mpcqp_create(int32_t n, int32_t m, const int32_t *Pp, const int32_t *Pi,
                 const int32_t *Ap, const int32_t *Ai, int64_t B,
                 const mpcqp_settings *settings, int32_t device, mpcqp_handle **out);
int mpcqp_setup_device(mpcqp_handle *h, const double *dPx, const double *dAx, const double *dq,
                       const double *dl, const double *du, void *stream);
int mpcqp_update_device(mpcqp_handle *h, const double *dq, const double *dl, const double *du,
                        void *stream);
int mpcqp_warm_start_device(mpcqp_handle *h, const double *dx, const double *dy, void *stream);
int mpcqp_solve_device(mpcqp_handle *h, double *dx, double *dy, int32_t *dstatus, int32_t *diters,
                       void *stream);
/* setup + warm start of the same call: mpcqp_setup_device(dPx..du) followed by
 * mpcqp_warm_start_device(dx0, dy0), with identical results (either may be null, as there).
 * Where mpcqp_setup_device takes the wide batch setup (the long-horizon plans: setup_wide.h;
 * not the plans of up to 256 columns and rows, which set up through setup_r.h) both run as ONE
 * kernel -- each workgroup scales its instance and forms x = D^-1 x0, y = E^-1 y0 c, z = A x
 * from the values still on chip -- so the warm-start kernel's pass over the workspace goes.
 * The reference's warm-started step prob.setup(...); prob.warm_start(x=, y=); prob.solve()
 * (mpc_dynamics.py:589-610 shifting the previous solution) maps onto it
 * followed by mpcqp_solve_device.  mpcqp_setup_warm_fused: 1 when the handle's plan takes the
 * one-kernel form, 0 when the call runs as the two launches. */
int mpcqp_setup_warm_device(mpcqp_handle *h, const double *dPx, const double *dAx, const double *dq,
                            const double *dl, const double *du, const double *dx0, const double *dy0,
                            void *stream);
int mpcqp_setup_warm_fused(const mpcqp_handle *h);
/* setup + solve of the same inputs in one call: mpcqp_setup_device(dPx..du) followed by
 * mpcqp_solve_device(dx, dy, dstatus, diters), with identical results.  Where the
 * solve kernel allows it -- the four-wave kernel k_setup_solve_w4 (the N=20 lateral
 * layouts: vanilla, and slack once its slack columns are eliminated) or the two-wave
 * kernel k_setup_solve_w2 -- both run as ONE kernel: each workgroup scales its instance
 * and solves it, so no setup kernel and no launch gap stand in front of the slowest
 * instance; the last workgroup also sorts the next dispatch order.  The reference's per-call
 * pattern prob.setup(...); prob.solve() (Control/MPC/mpc_kinematics.py:194-198,
 * mpc_dynamics.py:392-396) maps onto it one-to-one. */
int mpcqp_setup_solve_device(mpcqp_handle *h, const double *dPx, const double *dAx, const double *dq,
                             const double *dl, const double *du, double *dx, double *dy, int32_t *dstatus,
                             int32_t *diters, void *stream);
/* Gradients of the last solve's solution with respect to the problem data ("Gradients
 * of the solution"; not an osqp call).  For every instance whose status is "solved" and every
 * one of its nrhs seeds (g_x, g_y), with L = g_x . x + g_y . y, in the caller's units:
 *   row classes act[i]: 3 equality (l_i == u_i, always active), 1 lower (z_i - l_i < -y_i),
 *     2 upper (u_i - z_i < y_i) -- polish's rule on the workspace's scaled z and y --, 0 inactive;
 *   K [r_x; r_y] = [g_x; g_y] with K = [[P, A_act'], [A_act, 0]] over the active rows (g_y is read
 *     on active rows only; r_y = 0 on the others);
 *   gq = -r_x;  gl_i = r_y,i on a lower row, gu_i = r_y,i on an upper row, on an equality row
 *     r_y,i goes to gl_i when y_i <= 0 and to gu_i when y_i > 0; zero elsewhere and where the
 *     bound is infinite;
 *   gAx = -(y_i r_x,j + r_y,i x_j) per stored entry (i, j) of A;  gPx = -(r_x,i x_j + r_x,j x_i)
 *     per stored entry i < j of triu(P), -r_x,i x_i on the diagonal; both in the CSC order of the
 *     value arrays the setup took (per instance also in shared-matrix mode: the caller sums).
 * The linear solve is polish's: the settings' delta regularises, polish_refine_iter refinement
 * steps follow (both changeable through mpcqp_update_settings; settings.polish need not be on).
 * ares[b*nrhs + r] = ||K s - g||_inf / max(||g||_inf, tiny) on the scaled system after the last
 * step.  astat[b]: 0 the instance is not "solved" (every output of it is zero), 1 every seed's
 * ares is below 1e-8, -1 otherwise (K singular on the active set -- the slack layouts, whose
 * slack columns carry no quadratic cost -- or too ill-conditioned for the refinement steps
 * taken; a factorisation that fails or a solve that does not stay finite returns zeros with
 * ares = 1).  Seeds: gx (B, nrhs, n), gy (B, nrhs, m), either may be NULL (zeros), not both.
 * Outputs, any may be NULL: rx, gq (B, nrhs, n); ry, gl, gu (B, nrhs, m); gPx (B, nrhs, nnzP);
 * gAx (B, nrhs, nnzA); act (B, m); ares (B, nrhs); astat (B).
 * MPCQP_EINVAL: nrhs < 1, both seeds NULL, no solve since the last setup, or the workspace state
 * is gone (one-shot mode).  A handle whose plan eliminated variables moves to the plain plan
 * first, as under mpcqp_update_settings(polish = 1).  Like polish the call takes the workspace's
 * factor tiles (the next solve refactors) and leaves the iterates, the info and the statuses
 * alone.  mpcqp_adjoint_device: device pointers, enqueued on `stream` as mpcqp_solve_device.
 * mpcqp_adjoint_batch: host pointers, any handle of mpcqp_setup_batch (shards included), blocks
 * until the outputs are on the host. */
int mpcqp_adjoint_device(mpcqp_handle *h, int32_t nrhs, const double *dgx, const double *dgy, double *drx,
                         double *dry, double *dgq, double *dgl, double *dgu, double *dgPx, double *dgAx,
                         int8_t *dact, double *dares, int32_t *dastat, void *stream);
int mpcqp_adjoint_batch(mpcqp_handle *h, int32_t nrhs, const double *gx, const double *gy, double *rx, double *ry,
                        double *gq, double *gl, double *gu, double *gPx, double *gAx, int8_t *act, double *ares,
                        int32_t *astat);
/* The solution record: everything mpcqp_adjoint_* reads of a finished solve that a
 * setup does not rebuild.  n + 2m + 1 doubles per instance: the workspace's scaled iterates x~ (by
 * variable), z~, y~ and the status, exactly as mpcqp_adjoint_* reads them.  Opaque; meaningful only
 * to a handle of the same pattern whose current setup took the same data and settings the saving
 * one had (setup rebuilds the scaled data, D, E and c bit for bit from them).  Then
 *     mpcqp_setup_device(data); mpcqp_load_solution_device(record); mpcqp_adjoint_device(...)
 * returns, bit for bit, what the adjoint call right after the original solve returned -- act, ares
 * and astat included --, whatever the handle set up and solved in between: T differentiated solves
 * need one workspace and T records, not T workspaces.
 * save: one kernel on `stream`; needs a solve on the current setup (MPCQP_EINVAL as
 *   mpcqp_adjoint_device: no solve since the last setup, or the workspace state is gone in one-shot
 *   mode; also a NULL record).  A handle on an eliminated plan moves to the plain plan first, as
 *   under mpcqp_adjoint_device, so the record does not depend on the plan the solve ran on.
 * load: one kernel on `stream`; needs some setup on the handle (MPCQP_EINVAL before the first one,
 *   after a one-shot setup, for a NULL record) and makes the same plan move.  It writes the
 *   iterates and the statuses and marks the handle solved, so a following mpcqp_adjoint_* is
 *   defined; it touches nothing else: not the scaled data, not an instance's rho, not the info
 *   (obj, residuals, iteration counts, polish status, certificates stay those of the handle's last
 *   solve or setup).
 * A solve after a load is an ordinary solve of the current setup: with settings.warm_start on it
 * starts from the loaded x~, z~, y~ -- as after mpcqp_warm_start_device, but z~ is the record's
 * rather than A~ x~ -- at the rho the setup left (not the one the recorded solve had adapted to);
 * with warm_start off it starts from zero, as always.  It overwrites the loaded status. */
int mpcqp_save_solution_device(mpcqp_handle *h, double *drecord, void *stream);
int mpcqp_load_solution_device(mpcqp_handle *h, const double *drecord, void *stream);
/* LTI batches ("LTI shared-matrix mode"): with shared != 0 the following
 * mpcqp_setup_device / mpcqp_setup_solve_device calls read ONE Px[nnzP] and ONE Ax[nnzA]
 * for every instance of the batch instead of B copies (the lateral MPC's P and A do not
 * change between instances or steps: vehicle_lateral_mpc_slack_increment.py:79-115). */
int mpcqp_set_shared_matrices(mpcqp_handle *h, int32_t shared);
/* One-shot mode of mpcqp_setup_solve_device (the Control/MPC call pattern: a fresh OSQP()
 * + setup() + solve() every call, mpc_kinematics.py:194-198, so nothing reads the workspace
 * later): while on, the fused setup + solve kernel leaves the scaled problem on chip for the
 * solve instead of in the workspace, stores no warm-start iterates or certificates and keeps the
 * factorisation's G blocks on chip too where the plan leaves room (cfg 2, cfg 3) --
 * the outputs (x, y, status, iters) and the info are the same, bit for bit.  After such a call
 * the calls that read the workspace (update / warm_start / solve, the host batch calls, matrix
 * updates, certificates) fail with MPCQP_EINVAL until a setup.  mpcqp_one_shot_applies: 0 the
 * handle's kernel has no one-shot form (not the fused four-wave kernel, or polish: the call runs
 * as usual), 1 the form with the G blocks in the workspace, 2 with the G blocks in an LDS region
 * of their own, 3 with the G blocks written straight into the solve's LDS copy.
 * mpcqp_one_shot_kernel: which instantiation of the fused four-wave kernel a setup_solve on the
 * handle launches as currently set, as its GL number 0..5 (the form, the plan's
 * shape and MPCQP_ONE_SHOT_LOOP decide); -1 while one-shot mode is off, where no form applies,
 * for a NULL handle and for a sharded one.  The osqp API never turns one-shot mode on. */
int mpcqp_set_one_shot(mpcqp_handle *h, int32_t on);
int mpcqp_one_shot_applies(const mpcqp_handle *h);
int mpcqp_one_shot_kernel(const mpcqp_handle *h);
/* The handle's own hipStream_t (the one a NULL `stream` selects; first shard), so that a
 * caller's kernels (e.g. mpcqp_affine_apply_device) can be ordered with the handle's calls. */
void *mpcqp_get_stream(const mpcqp_handle *h);
/* Blocks until every call enqueued on the handle so far has finished, on the handle's
 * own stream(s) and on the caller stream the last *_device call used. */
int mpcqp_synchronize(mpcqp_handle *h);
/* hipEvent-bracketed time of the last solve: milliseconds, or -1 when unavailable.
 * Recorded only while mpcqp_timing is on, by the host-pointer mpcqp_solve_batch and the
 * *_device entry points alike (no event packet between the kernels otherwise). */
double mpcqp_last_kernel_ms(mpcqp_handle *h);

/* Kernel timing for bench.py's roofline: while enabled, every *_device solve
 * (enable bit 0) / setup (bit 1) launch is bracketed by a hipEvent pair on its
 * stream (no host sync).  mpcqp_timing_read() waits for the recorded events,
 * returns the summed kernel milliseconds and launch counts, and clears the
 * record. */
int mpcqp_timing(mpcqp_handle *h, int32_t enable);
int mpcqp_timing_read(mpcqp_handle *h, double *setup_ms, int32_t *n_setup, double *solve_ms,
                      int32_t *n_solve);

int mpcqp_get_plan_info(const mpcqp_handle *h, mpcqp_plan_info *info);
/* Diagnostics: per-instance phase timers of the last solve (24 int64 per instance:
 * factor, rhs, bt_solve, update, checks, tail shader-clock cycles, total cycles,
 * total 100 MHz wall ticks, then the factorisation split: assembly, F/S products,
 * Gauss-Jordan, block epilogue, then the block-solve split of the wave kernels:
 * phase A, B, C, spare, then eight per-wave sub-phase times of the long-horizon kernel).  Only when MPCQP_PHASE_PROF=1 was set at creation. */
int mpcqp_debug_phase_times(mpcqp_handle *h, int64_t *out);
/* Diagnostics: the dispatch order the next solve will use (B int32 instance indices, each
 * shard's own order offset by its first instance): after a solve, that solve's instances by
 * descending iteration bucket (iter >> shift, 256 buckets; order within a bucket is not
 * fixed).  Sorted in the solve kernel's last workgroup (four- and two-wave kernels) or by
 * k_order (MPCQP_ORDER_KERNEL=1 at creation); identity before the first solve and under
 * MPCQP_DISPATCH=identity. */
int mpcqp_debug_dispatch_order(mpcqp_handle *h, int32_t *out);
/* Diagnostics (bench.py's achievable-HBM reference): `reps` device-to-device
 * copies of n doubles (n a multiple of 16384; 16-byte aligned buffers) by a streaming copy
 * kernel -- 16-byte loads and stores, four or eight in flight per lane, 256-thread workgroups;
 * five forms (non-temporal; default policy; default policy with eight per lane; one pass of a
 * workgroup per 16 KiB, default policy or non-temporal) -- on `stream`
 * (hipStream_t, NULL: the null stream of the current device; a non-NULL stream makes its own
 * device the calling thread's current one), timed by an event pair around each form's launches:
 * *ms = the average per copy of the fastest form.  Blocks until done. */
int mpcqp_debug_copy(const double *src, double *dst, int64_t n, int32_t reps, void *stream, double *ms);

void mpcqp_free(mpcqp_handle *h);
const char *mpcqp_last_error(void);

/* Host-only symbolic analysis (no device needed): block-tridiagonal plan of
 * K = P + sigma I + A' diag(rho) A.  var_pad[n] receives each variable's padded
 * index, bsize[*nb] the block sizes (capacity n).  Used by the CPU test-suite. */
int mpcqp_analyze(int32_t n, int32_t m, const int32_t *Pp, const int32_t *Pi,
                  const int32_t *Ap, const int32_t *Ai, int32_t *nb, int32_t *block,
                  int32_t *var_pad, int32_t *bsize);
/* Same, with `eliminate`: the plan a handle uses for the four-wave kernel -- degree <= 1
 * vertices of K's graph (slack columns) taken out of the blocks (padded indices from
 * nb * block on), blocks packed greedily; n_eliminated (may be NULL) receives their count. */
int mpcqp_analyze_ex(int32_t n, int32_t m, const int32_t *Pp, const int32_t *Pi,
                     const int32_t *Ap, const int32_t *Ai, int32_t eliminate, int32_t *nb,
                     int32_t *block, int32_t *var_pad, int32_t *bsize, int32_t *n_eliminated);

/* Host-only (no device needed): the plan and solve-kernel variant a handle created with
 * this pattern and these settings (NULL: defaults) would take -- the shape fields of
 * mpcqp_plan_info (batch, n_devices = 0) -- and, in note[note_cap] (may be NULL), why an
 * eliminated plan was rejected ("" otherwise).  Used by the CPU test-suite to pin the
 * kernel shape of each workload (e.g. the slack layout's reduced system: 4 blocks, amax <= 8). */
int mpcqp_plan_preview(int32_t n, int32_t m, const int32_t *Pp, const int32_t *Pi,
                       const int32_t *Ap, const int32_t *Ai, const mpcqp_settings *settings,
                       mpcqp_plan_info *info, char *note, int32_t note_cap);

/* ======================================================================
 * The MPC data path around the solver, on the device.
 * Replaces the Python work of Control/MPC/mpc_dynamics.py:main between two
 * osqp solves, batched over B vehicles.  Device pointers, enqueued on `stream`.
 * ====================================================================== */

/* Vehicle_Dynamics(...) constructor arguments (Vehicle_Dynamics/vehicle_models.py:27-50) */
typedef struct {
    double m, l_f, l_r, width, length, C_d, A_f, C_roll, dt;
} mpcqp_vehicle;

/* F2 -- Vehicle_Dynamics.get_dynamics_model (vehicle_models.py:52-340), batched.
 * For b < B, k < N: x = dx[b*x_sb + k*x_sk + 0..6) = (X, Y, yaw, vx, vy, r),
 * u = du[b*u_sb + k*u_sk + 0..2) = (steer, accel)  ->  Ad[(b*N + k)*36] (6x6),
 * Bd[(b*N + k)*12] (6x2), gd[(b*N + k)*6], row-major.  The low-speed guard
 * (:143-159) acts on copies: unlike the reference, inputs are never written. */
int mpcqp_linearise_device(const mpcqp_vehicle *veh, int64_t B, int32_t N, const double *dx, int64_t x_sb,
                           int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk, double *dAd, double *dBd,
                           double *dgd, int32_t device, void *stream);

/* F1 -- the QP of mpc_increment (Control/MPC/mpc_dynamics.py:281-389) for a batch
 * sharing N, nx, nu, weights, bounds and the structural nonzeros of Ad / Bd
 * (maskA[nx*nx], maskB[nx*nu], 1 = entry may be nonzero).  Q, QN (nx x nx) and
 * R (nu x nu) are dense row-major; xmin_t / xmax_t have nx+nu entries, dumin /
 * dumax nu (+-inf allowed; clipped to +-1e30 as the osqp wrapper does).
 * Variables (x~_0..x~_N, du_0..du_{N-1}), x~ = (x, u_prev); rows [A_eq; I]. */
typedef struct mpcqp_incr_layout mpcqp_incr_layout;
int mpcqp_incr_layout_create(int32_t N, int32_t nx, int32_t nu, const double *Q, const double *QN, const double *R,
                             const double *xmin_t, const double *xmax_t, const double *dumin, const double *dumax,
                             const uint8_t *maskA, const uint8_t *maskB, int32_t device, mpcqp_incr_layout **out);
int mpcqp_incr_layout_dims(const mpcqp_incr_layout *L, int32_t *n, int32_t *m, int32_t *nnzP, int32_t *nnzA);
/* The shared pattern (P upper-triangular CSC with its constant values; A CSC) and the
 * constant parts of the per-instance arrays; any pointer may be NULL. */
int mpcqp_incr_layout_pattern(const mpcqp_incr_layout *L, int32_t *Pp, int32_t *Pi, double *Px, int32_t *Ap,
                              int32_t *Ai, double *Ax_template, double *l_template, double *u_template);
/* Per instance b: Ad/Bd/gd as produced by mpcqp_linearise_device for stages 0..N-1,
 * xt0[b*(nx+nu)] = x~(0), Xr[b*nx*(N+1)] = reference (nx rows, N+1 columns)
 * -> Ax[b*nnzA], q[b*n], l[b*m], u[b*m] for mpcqp_setup_device. */
int mpcqp_incr_assemble_device(const mpcqp_incr_layout *L, int64_t B, const double *dAd, const double *dBd,
                               const double *dgd, const double *dxt0, const double *dXr, double *dAx, double *dq,
                               double *dl, double *du, void *stream);
void mpcqp_incr_layout_free(mpcqp_incr_layout *L);

/* F1 for the LTI lateral layouts (vehicle_lateral_mpc_slack_increment.py:32-121 and its loop
 * :201-229; Control/MPC/mpc_kinematics.py:148-191 with the lateral model): their P and A
 * are the same for every instance and step (mpcqp_set_shared_matrices), and every entry of
 * the concatenated (q | l | u) is affine in the instance's parameters theta = (x0, xr) with
 * a base vector per bound regime (the script's i <= 400 / <= 900 / else schedule, :158-172):
 *     v[i] = base[regime][i] + sum_{t < T} coef[i*T + t] * theta[idx[i*T + t]]   (idx -1: none)
 * The map is built once on the host from the layout's builder (osqp_amd.mpc_device.
 * LateralAssembler); mpcqp_affine_apply_device then writes q[B*seglen0], l[B*seglen1],
 * u[B*seglen2] from theta[b*theta_stride + k] and regime[b] (NULL: regime 0; clamped to
 * [0, nregimes)), one thread per (instance, entry).  An entry with terms is the terms' sum
 * (plus its base where that is nonzero), so a product the builder forms alone is exact. */
typedef struct mpcqp_affine mpcqp_affine;
int mpcqp_affine_create(int32_t nseg, const int32_t *seglen, int32_t nregimes, int32_t T, const double *base,
                        const int32_t *idx, const double *coef, int32_t device, mpcqp_affine **out);
int mpcqp_affine_apply_device(const mpcqp_affine *a, int64_t B, const double *dtheta, int32_t theta_stride,
                              const int32_t *dregime, double *dout0, double *dout1, double *dout2, void *stream);
void mpcqp_affine_free(mpcqp_affine *a);

/* F3 -- reference_search (mpc_dynamics.py:44-90, nearest_point :30-41) for every
 * vehicle: pred[b*(N+1)*nxa + k*nxa + 0..nxa) predicted augmented states
 * -> Xr[b*6*(N+1)] (6 rows: path x, path y, yaw 0, vx 10, vy 0, r 0).  Near the
 * path's end the index holds the start of the last segment (where the reference
 * raises IndexError). */
int mpcqp_reference_search_device(int64_t B, int32_t N, int32_t nxa, int32_t npath, const double *dpath_x,
                                  const double *dpath_y, const double *dpred, double dt, double *dXr, int32_t device,
                                  void *stream);
/* F3 -- plant step and horizon shift of mpc_dynamics.main (:578-617), dynamic bicycle
 * (nx 6, nu 2): from the unscaled solutions sol[b*n] and the step's stage-0 model
 * (Ad/Bd/gd of mpcqp_linearise_device), advance x~ (xt[b*8], in/out) and write the
 * shifted predictions pred[b*(N+1)*8] and pred_du[b*(N+1)*2]. */
int mpcqp_incr_shift_device(const mpcqp_incr_layout *L, const mpcqp_vehicle *veh, int64_t B, const double *dsol,
                            const double *dAd, const double *dBd, const double *dgd, double *dxt, double *dpred,
                            double *dpdu, void *stream);
/* The transpose of mpcqp_incr_shift_device as it computes: cotangents dgxt[b*8],
 * dgpred[b*(N+1)*8], dgpdu[b*(N+1)*2] of the NEW xt, pred, pred_du (each may be NULL = zero) ->
 * dgsol[b*n], the stage-0 model's dgAd0[b*36], dgBd0[b*12], dggd0[b*6] (the caller adds them into
 * stage 0 of the linearisation's cotangents) and dgxt_before[b*8]; a NULL output is not written.
 * dsol, dAd, dBd as the forward took them (stage 0 of dAd / dBd is read; dgd is not read -- the step
 * is affine in it -- and may be NULL); dxt_before is x~ from BEFORE the step, which the forward
 * overwrote.  The plant step is bilinear; the shift is copies, and where the forward wrote one
 * source twice (pred_du[N-1] and [N]; the inputs of pred[N-1] and [N]) the cotangents add; the
 * terminal state is differentiated as mpcqp_linearise_vjp_device differentiates the linearisation:
 * the low-speed guard first (vy, r, steer carry nothing for |vx| < 0.5, vx nothing for |vx| < 0.3,
 * exactly), then the Euler step of the same tyre and dynamics functions over forward-mode duals;
 * sgn(vx) has derivative 0.  One writer per output element, no atomics: a repeated call returns
 * the same bits.  MPCQP_EINVAL "incr_shift_vjp: bad arguments" (a NULL layout, vehicle, dsol, dAd,
 * dBd or dxt_before, B < 0) and MPCQP_EUNSUPPORTED (a layout that is not nx 6, nu 2) before any
 * device call. */
int mpcqp_incr_shift_vjp_device(const mpcqp_incr_layout *L, const mpcqp_vehicle *veh, int64_t B, const double *dsol,
                                const double *dAd, const double *dBd, const double *dgd, const double *dxt_before,
                                const double *dgxt, const double *dgpred, const double *dgpdu, double *dgsol,
                                double *dgAd0, double *dgBd0, double *dggd0, double *dgxt_before, void *stream);
/* F3 -- warm start for the next step (cfg 5): shift a solution of
 * the incremental layout one stage forward, x[b*n], y[b*m] -> xs[b*n], ys[b*m].
 * Variable blocks x~_0..x~_N | du_0..du_{N-1} and row blocks eq_0..eq_N |
 * box_0..box_N | du-box_0..du-box_{N-1} each move k+1 -> k, the last one repeated
 * (the reference's own shift of pred_x~ / pred_du, mpc_dynamics.py:589-610, applied
 * to the primal and dual iterates).  y / ys may be NULL.  In-place is not allowed. */
int mpcqp_incr_warm_shift_device(int64_t B, int32_t N, int32_t nxa, int32_t nu, const double *dx, const double *dy,
                                 double *dxs, double *dys, int32_t device, void *stream);

/* ======================================================================
 * The same loop on the kinematic bicycle: Control/MPC/mpc_incre_kine_func.py
 * simulate (:223-436), batched.  State (x, y, v, yaw), input (steer, accel);
 * the QP is mpcqp_incr_layout with nx 4, nu 2 (mpcqp_incr_assemble_device).
 * ====================================================================== */

/* Vehicle_Kinematics(...) constructor arguments (vehicle_models.py:829-833) */
typedef struct {
    double l_f, l_r, dt;
} mpcqp_kin_vehicle;

/* Vehicle_Kinematics.get_kinematics_model (vehicle_models.py:835-863), batched.
 * For b < B, k < N: x = dx[b*x_sb + k*x_sk + 0..4), u = du[b*u_sb + k*u_sk + 0..2)
 * -> Ad[(b*N + k)*16] (4x4), Bd[(b*N + k)*8] (4x2), gd[(b*N + k)*4], row-major.
 * Inputs are never written. */
int mpcqp_kin_linearise_device(const mpcqp_kin_vehicle *veh, int64_t B, int32_t N, const double *dx, int64_t x_sb,
                               int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk, double *dAd, double *dBd,
                               double *dgd, int32_t device, void *stream);

/* reference_search (mpc_incre_kine_func.py:42-81, nearest_point :28-40, look_ind 1) for
 * every vehicle: pred[b*(N+1)*nxa + k*nxa + 0..nxa) (speed in state 2), path_x / path_y /
 * path_yaw[npath], set_speed[B] -> Xr[b*4*(N+1)] (4 rows: path x, path y, set_speed[b],
 * path_yaw at the same index).  Near the path's end the index holds the start of the last
 * segment (where the reference raises IndexError), as mpcqp_reference_search_device does. */
int mpcqp_kin_reference_search_device(int64_t B, int32_t N, int32_t nxa, int32_t npath, const double *dpath_x,
                                      const double *dpath_y, const double *dpath_yaw, const double *dset_speed,
                                      const double *dpred, double dt, double *dXr, int32_t device, void *stream);

/* The tail of simulate's loop (:382-428) for a layout with nx 4, nu 2 (any other:
 * MPCQP_EUNSUPPORTED).  Per vehicle b with done[b] == 0, in the reference's order:
 *   1. unpack sol[b*n] as mpc_increment does (:194-217);
 *   2. while traj_len[b] < traj_cap, append (x, y, yaw, du_0[steer]) of the state the step
 *      started from to traj[(b*traj_cap + traj_len[b])*4] and count it (:389-393);
 *   3. stop rule (:395-401): if the distance from that state to Xr[:, 0] is below 0.5,
 *      finish_cnt[b] goes up; once it exceeds 15, done[b] = 1, pred / pred_du hold the
 *      unpacked solution (the reference breaks right after mpc_increment wrote them) and
 *      nothing below runs;
 *   4. plant step u = u_prev + du_0, x+ = Ad_0 x + Bd_0 u + gd_0 into xt[b*6];
 *   5. horizon shift (:407-428) into pred[b*(N+1)*6], pred_du[b*(N+1)*2].  The reference
 *      shifts in place, so its terminal Euler step (update_kinematics_model) takes the
 *      solution's stage-N state AND stage-N control, and advances v before yaw uses it.
 * A vehicle with done[b] != 0 is left untouched (xt, pred, pred_du, finish_cnt, traj).
 * traj / traj_len may be NULL when traj_cap is 0.  finish_cnt, done, traj_len: int32[B]. */
int mpcqp_kin_shift_device(const mpcqp_incr_layout *L, const mpcqp_kin_vehicle *veh, int64_t B, const double *dsol,
                           const double *dAd, const double *dBd, const double *dgd, const double *dXr, double *dxt,
                           double *dpred, double *dpdu, int32_t *dfinish_cnt, int32_t *ddone, double *dtraj,
                           int32_t traj_cap, int32_t *dtraj_len, void *stream);

/* ======================================================================
 * The LTV MPC in the inputs themselves (no u_prev augmentation): the layout of
 * Control/MPC/mpc_kinematics_pred_matrix.py:268-352 mpc__, mpc_dynamics.py:160-279 mpc and
 * mpc_kinematics.py:202-265 mpc_ (per-stage state bounds), and the closed loop of
 * mpc_kinematics_pred_matrix.main (:355-563).
 * ====================================================================== */

/* Variables (x_0..x_N, u_0..u_{N-1}): n = (N+1) nx + N nu; rows [A_eq; I]: (N+1) nx dynamics
 * equalities, then the identity box on every variable, m = 2 (N+1) nx + N nu.
 * P = blockdiag(Q x N, QN, R x N) (upper-triangular CSC, constant); A_eq = -I on the diagonal,
 * Ad_k on the sub-diagonal, Bd_k one block down, its pattern from maskA[nx*nx] / maskB[nx*nu]
 * as in mpcqp_incr_layout.  Q, QN (nx x nx), R (nu x nu) dense row-major; xmin / xmax nx
 * entries, umin / umax nu (+-inf allowed, clipped to +-1e30).  N >= 2, 1 <= nx <= 6,
 * 1 <= nu <= 2, else MPCQP_EUNSUPPORTED. */
typedef struct mpcqp_ltv_layout mpcqp_ltv_layout;
int mpcqp_ltv_layout_create(int32_t N, int32_t nx, int32_t nu, const double *Q, const double *QN, const double *R,
                            const double *xmin, const double *xmax, const double *umin, const double *umax,
                            const uint8_t *maskA, const uint8_t *maskB, int32_t device, mpcqp_ltv_layout **out);
int mpcqp_ltv_layout_dims(const mpcqp_ltv_layout *L, int32_t *n, int32_t *m, int32_t *nnzP, int32_t *nnzA);
/* As mpcqp_incr_layout_pattern; any pointer may be NULL. */
int mpcqp_ltv_layout_pattern(const mpcqp_ltv_layout *L, int32_t *Pp, int32_t *Pi, double *Px, int32_t *Ap,
                             int32_t *Ai, double *Ax_template, double *l_template, double *u_template);
/* Per instance b: Ad[b*N*nx*nx], Bd[b*N*nx*nu], gd[b*N*nx] for stages 0..N-1, x0[b*nx],
 * Xr[b*nx*(N+1)] (nx rows, N+1 columns) -> Ax[b*nnzA], q[b*n] = (-Q Xr_k (k < N); -QN Xr_N; 0),
 * l[b*m], u[b*m] with l = u = (-x0; -gd_k) on the equality rows.  xlo / xhi[b*(N+1)*nx]
 * (stage-major) are optional per-instance, per-stage state bounds (the corridor of mpc_):
 * NULL = the layout's xmin / xmax on every stage; given, they replace the state rows of the
 * box, clipped to +-1e30.  The input rows of the box always come from the layout. */
int mpcqp_ltv_assemble_device(const mpcqp_ltv_layout *L, int64_t B, const double *dAd, const double *dBd,
                              const double *dgd, const double *dx0, const double *dXr, const double *dxlo,
                              const double *dxhi, double *dAx, double *dq, double *dl, double *du, void *stream);
void mpcqp_ltv_layout_free(mpcqp_ltv_layout *L);

/* Initial horizon of mpc_kinematics_pred_matrix.main (:405-419): pred_u[b*(N+1)*2] = u0[b*2]
 * in all N+1 stages, pred_x[b*(N+1)*4]: stage 0 = x0[b*4], stage k+1 =
 * update_kinematics_model(stage k, u0) (vehicle_models.py:866-883: the nonlinear Euler step,
 * v advanced before yaw reads it). */
int mpcqp_kin_rollout_device(const mpcqp_kin_vehicle *veh, int64_t B, int32_t N, const double *dx0,
                             const double *du0, double *dpred_x, double *dpred_u, int32_t device, void *stream);

/* The tail of mpc_kinematics_pred_matrix.main's loop (:479-563) for a layout with nx 4, nu 2
 * (any other: MPCQP_EUNSUPPORTED).  sol[b*n] = (S_0..S_N, U_0..U_{N-1}).  status[b] is the
 * solver's code (NULL: all solved).  A vehicle whose status is not 1 (solved) is skipped as
 * the reference's `continue` skips it: x, u, pred_x, pred_u, traj, traj_len and steps_taken
 * stay bit for bit and skipped[b] goes up.  Otherwise:
 *   1. while traj_len[b] < traj_cap, append (x, y, v, yaw, U_0[steer], U_0[accel]) -- the
 *      state the step started from and the control applied -- to
 *      traj[(b*traj_cap + traj_len[b])*6] and count it;
 *   2. plant step x <- Ad_0 x + Bd_0 U_0 + gd_0 (x[b*4]), u <- U_0 (u[b*2]);
 *   3. pred_x: stage 0 = x, stage k = S_{k+1} (1 <= k <= N-1), stage N =
 *      update_kinematics_model(S_N, U_{N-1});
 *   4. pred_u: stage k = U_{k+1} (k <= N-2), stages N-1 and N = U_{N-1};
 *   5. steps_taken[b] goes up.
 * skipped, steps_taken, traj_len: int32[B]; steps_taken may be NULL, traj / traj_len when
 * traj_cap is 0. */
int mpcqp_kin_ltv_shift_device(const mpcqp_ltv_layout *L, const mpcqp_kin_vehicle *veh, int64_t B,
                               const double *dsol, const int32_t *dstatus, const double *dAd, const double *dBd,
                               const double *dgd, double *dx, double *du, double *dpred_x, double *dpred_u,
                               int32_t *dskipped, int32_t *dsteps_taken, double *dtraj, int32_t traj_cap,
                               int32_t *dtraj_len, void *stream);

/* The transposes of the two kinematic tails as they compute, for a layout with
 * nx 4, nu 2.  dmode[b] (int32[B]; NULL: 0 for every vehicle) says what the forward did:
 *   0  the vehicle was stepped;
 *   1  the forward left it untouched (mpcqp_kin_shift_device: done[b] was already set;
 *      mpcqp_kin_ltv_shift_device: status[b] != 1): dgsol and the model outputs are exactly zero
 *      and the state's cotangent passes through (dgxt_before = dgxt, dgx_before = dgx);
 *   2  mpcqp_kin_shift_device only: the vehicle met the stop rule on this step (finish_cnt went
 *      past 15), so pred / pred_du hold the unpacked solution and xt did not move:
 *      g x~_k = dgpred[k] for all k, g du_k = dgpdu[k], du_{N-1} also takes dgpdu[N],
 *      dgxt_before = dgxt, the model outputs are zero.
 * Left to the caller: the cotangent of the PREVIOUS pred / pred_du (pred_x, pred_u and u for the
 * LTV tail), which is dgpred / dgpdu (dgpred_x, dgpred_u, dgu) in mode 1 and zero in modes 0 and 2;
 * these calls do not write it.
 *
 * mpcqp_kin_shift_vjp_device, mode 0, with w = dgxt + dgpred[0] and u = u_prev + du_0:
 *   dgAd0[b*16] = w_x x',  dgBd0[b*8] = w_x u',  dggd0[b*4] = w_x,  g u = w_u + Bd0' w_x,
 *   dgxt_before[b*6] = (Ad0' w_x, g u),  g du_0 = g u;
 *   g x~_k = dgpred[k-1] (2 <= k <= N),  g du_k = dgpdu[k-1] (1 <= k <= N-1),  du_{N-1} also takes
 *   dgpdu[N-1] and dgpdu[N], in that order;  x~_0 and x~_1 get nothing;
 *   the forward's terminal state is (update_kinematics_model(x_N, u_N), u_N) of x~_N's own two
 *   parts, so x~_N also takes dgpred[N]'s input part and the closed-form transpose of the update
 *   applied to dgpred[N]'s state part.
 * mpcqp_kin_ltv_shift_vjp_device, mode 0, with w = dgx + dgpred_x[0]:
 *   dgAd0 = w x',  dgBd0 = w U_0',  dggd0 = w,  dgx_before[b*4] = Ad0' w,  g U_0 = Bd0' w + dgu
 *   (the forward does not read the old u);  g S_k = dgpred_x[k-1] (2 <= k <= N),  g U_k =
 *   dgpred_u[k-1] (1 <= k <= N-1),  U_{N-1} also takes dgpred_u[N-1] and dgpred_u[N];  the terminal
 *   update is of (S_N, U_{N-1}): its transpose of dgpred_x[N] goes into S_N and U_{N-1}.
 * dsol, dAd, dBd as the forward took them (stage 0 of dAd / dBd is read; dgd is not read and may
 * be NULL); dxt_before / dx_before is the state from BEFORE the step.  Each cotangent may be NULL
 * (zero), each output may be NULL (not written).  One thread per (vehicle, output row), one writer
 * per element, no atomics: a repeated call returns the same bits.  MPCQP_EINVAL "kin_shift_vjp: bad
 * arguments" / "kin_ltv_shift_vjp: bad arguments" (a NULL layout, vehicle, dsol, dAd, dBd or
 * state-before, B < 0) and MPCQP_EUNSUPPORTED (a layout that is not nx 4, nu 2) before any device
 * call; B == 0 or no output asked for succeeds without one. */
int mpcqp_kin_shift_vjp_device(const mpcqp_incr_layout *L, const mpcqp_kin_vehicle *veh, int64_t B, const double *dsol,
                               const double *dAd, const double *dBd, const double *dgd, const double *dxt_before,
                               const int32_t *dmode, const double *dgxt, const double *dgpred, const double *dgpdu,
                               double *dgsol, double *dgAd0, double *dgBd0, double *dggd0, double *dgxt_before,
                               void *stream);
int mpcqp_kin_ltv_shift_vjp_device(const mpcqp_ltv_layout *L, const mpcqp_kin_vehicle *veh, int64_t B,
                                   const double *dsol, const double *dAd, const double *dBd, const double *dx_before,
                                   const int32_t *dmode, const double *dgx, const double *dgu, const double *dgpred_x,
                                   const double *dgpred_u, double *dgsol, double *dgAd0, double *dgBd0, double *dggd0,
                                   double *dgx_before, void *stream);

/* ======================================================================
 * A bank of paths with a per-vehicle selection, and the two closed loops built on the layouts
 * above that remain in Control/MPC: mpc_increment_kinematics_pred_matrix.main (:281-476, the
 * double lane change) and mpc_kinematics.main (:268-461, one linearisation per step).
 * ====================================================================== */

/* mpcqp_kin_reference_search_device over `npaths` paths of npath points each: path p is
 * paths_x / paths_y / paths_yaw[p*npath .. (p+1)*npath), and vehicle b walks path path_id[b]
 * (int32[B]; NULL: path 0 for every vehicle).  A path_id outside [0, npaths) never indexes the
 * bank: it is clamped to the nearest valid path (negative -> 0, too large -> npaths - 1).
 * paths_yaw may be NULL: row 3 of Xr is then 0 on every point (the reference_search of
 * mpc_increment_kinematics_pred_matrix.py:41-83 and mpc_kinematics.py:39-81).  The nearest-point
 * search, the walk and the hold of the last segment are those of the one-path entry point; with
 * npaths = 1 and path_id = NULL the output equals its output bit for bit. */
int mpcqp_kin_reference_search_paths_device(int64_t B, int32_t N, int32_t nxa, int32_t npaths, int32_t npath,
                                            const double *dpaths_x, const double *dpaths_y, const double *dpaths_yaw,
                                            const int32_t *dpath_id, const double *dset_speed, const double *dpred,
                                            double dt, double *dXr, int32_t device, void *stream);

/* The tail of mpc_increment_kinematics_pred_matrix.main's loop (:423-472) for an incremental
 * layout with nx 4, nu 2 (any other: MPCQP_EUNSUPPORTED; so is nsw > 8).  switch_steps[nsw] and
 * paths_of[nsw + 1] are HOST arrays (the convention of mpcqp_lti_step_device); everything else
 * is on the device.  There is no skip rule: mpc_increment uses the solution whatever the
 * solver's status (:248-252).  Per vehicle b, in the reference's order:
 *   1. while traj_len[b] < traj_cap, append (x, y, v, yaw, steer, accel) of xt[b*6] as the step
 *      started -- plt_states / plt_actions, :423-424: the input is the one held BEFORE the
 *      step -- to traj[(b*traj_cap + traj_len[b])*6] and count it;
 *   2. plant step u = u_prev + du_0, x+ = Ad_0 x + Bd_0 u + gd_0 into xt[b*6] (:442-449);
 *   3. horizon shift (:451-472) into pred[b*(N+1)*6], pred_du[b*(N+1)*2], as step 5 of
 *      mpcqp_kin_shift_device (the same text in the reference: the terminal Euler step takes the
 *      solution's stage-N state and stage-N control, v advanced before yaw reads it);
 *   4. step[b] += 1, then path_id[b] = paths_of[#{j < nsw : step[b] > switch_steps[j]}]: the
 *      path the NEXT step's reference search runs on (the script, sim_time 1000: switch_steps
 *      (50, 150), paths_of (0, 1, 0), :380-391).  paths_of is not range-checked here; the
 *      search clamps.
 * step, path_id, traj_len: int32[B].  traj / traj_len may be NULL when traj_cap is 0. */
int mpcqp_lane_tail_device(const mpcqp_incr_layout *L, const mpcqp_kin_vehicle *veh, int64_t B, const double *dsol,
                           const double *dAd, const double *dBd, const double *dgd, double *dxt, double *dpred,
                           double *dpdu, int32_t nsw, const int32_t *switch_steps, const int32_t *paths_of,
                           int32_t *dstep, int32_t *dpath_id, double *dtraj, int32_t traj_cap, int32_t *dtraj_len,
                           void *stream);

/* The tail of mpc_kinematics.main's loop (:397-456) for an LTV layout with nx 4, nu 2 (any
 * other: MPCQP_EUNSUPPORTED).  sol[b*n] = (S_0..S_N, U_0..U_{N-1}); Ad[b*N*16], Bd[b*N*8],
 * gd[b*N*4] are the lists the assembly took, of which stage 0 is read (the loop uses one model,
 * linearised at the current (x, u), on every stage).  status[b] is the solver's code (NULL: all
 * solved).  A vehicle whose status is not 1 (solved) is skipped as the reference's `continue`
 * skips it (:398-402): x, u, pred_x, traj, traj_len and steps_taken stay bit for bit and
 * skipped[b] goes up.  Otherwise:
 *   1. pred_x[b*(N+1)*4]: stage k = S_k for every k = 0..N (stage 0 is the solution's, not the
 *      plant state; there is no shift, :410-420);
 *   2. while traj_len[b] < traj_cap, append (x, y, v, yaw, U_0[steer], U_0[accel]) -- the state
 *      the step started from and the control applied (:452-453) -- to
 *      traj[(b*traj_cap + traj_len[b])*6] and count it;
 *   3. plant step x <- Ad_0 x + Bd_0 U_0 + gd_0 (x[b*4]), u <- U_0 (u[b*2]);
 *   4. steps_taken[b] goes up.
 * skipped, steps_taken, traj_len: int32[B]; steps_taken may be NULL, traj / traj_len when
 * traj_cap is 0. */
int mpcqp_kin_frozen_tail_device(const mpcqp_ltv_layout *L, int64_t B, const double *dsol, const int32_t *dstatus,
                                 const double *dAd, const double *dBd, const double *dgd, double *dx, double *du,
                                 double *dpred_x, int32_t *dskipped, int32_t *dsteps_taken, double *dtraj,
                                 int32_t traj_cap, int32_t *dtraj_len, void *stream);

/* ======================================================================
 * The closed loop that keeps one problem alive: vehicle_lateral_mpc_slack_increment.py
 * (setup once :121, then per step update(q=, l=, u=) :237 and a warm-started solve :248).
 * q, l, u come from mpcqp_affine_apply_device, the update and the solve from
 * mpcqp_update_device / mpcqp_solve_device; this is the tail of the loop (:252-269).
 * ====================================================================== */

/* For any LTI model x~+ = At x~ + Bt du with nxa <= 8 states and 1 <= nu <= min(2, nxa) inputs
 * (else MPCQP_EUNSUPPORTED; so is nsw > 8).  At (nxa x nxa) and Bt (nxa x nu) are HOST arrays,
 * row-major; switch_steps[nsw] and regimes[nsw + 1] are HOST arrays too.  Everything else is
 * on the device: sol[b*n] with du_0[j] = sol[b*n + du_off + j] and the recorded slack
 * sol[b*n + slack_off] (slack_off < 0: none, 0 is recorded), status[b] the solver's code,
 * x~ of vehicle b at xt[b*xt_stride .. + nxa) (in/out), and int32[B] step, regime, failed,
 * fail_step, traj_len.
 *
 * A vehicle with failed[b] != 0 is left untouched.  If status[b] != MPCQP_SOLVED (`solved
 * inaccurate` included) -- the script's raise, :252-253 -- failed[b] = 1, fail_step[b] = step[b]
 * and nothing else of the vehicle changes, on this call or any later one.  Otherwise:
 *   1. while traj_len[b] < traj_cap, append a row of nxa + nu + 1 doubles to
 *      traj[(b*traj_cap + traj_len[b])*(nxa + nu + 1)] and count it: the first nxa - nu states
 *      BEFORE the step, the last nu states AFTER it, du_0, the slack (the script's plt_x_1..4,
 *      plt_u, plt_del_u, plt_s);
 *   2. plant step, every product and every sum rounded on its own (no fused multiply-add), per
 *      row i:  acc = At[i][0] x[0];  acc = acc + At[i][j] x[j] for j = 1..nxa-1 in order;
 *      bu = Bt[i][0] du[0] (+ Bt[i][1] du[1]);  x+[i] = acc + bu  -- the order
 *      osqp_amd.mpc.lti_step restates on the host, bit for bit;
 *   3. step[b] += 1, then regime[b] = regimes[#{j < nsw : step[b] > switch_steps[j]}]: the
 *      regime the NEXT step assembles with (the script: switch_steps (400, 900), regimes
 *      (0, 1, 0), :158-172).
 * traj / traj_len may be NULL when traj_cap is 0. */
int mpcqp_lti_step_device(int64_t B, int32_t nxa, int32_t nu, const double *At, const double *Bt, int32_t n,
                          int32_t du_off, int32_t slack_off, const double *dsol, const int32_t *dstatus, double *dxt,
                          int64_t xt_stride, int32_t nsw, const int32_t *switch_steps, const int32_t *regimes,
                          int32_t *dstep, int32_t *dregime, int32_t *dfailed, int32_t *dfail_step, double *dtraj,
                          int32_t traj_cap, int32_t *dtraj_len, int32_t device, void *stream);

/* ======================================================================
 * The MPC step differentiated: vector-Jacobian products of the assembly of both
 * layouts, of the affine lateral assembler and of the kinematic linearisation, and the assembly
 * with weights given per call.  Chained after mpcqp_adjoint_device they give d(solution) /
 * d(x0, Xr, Q, QN, R, Ad, Bd, gd, x, u).  Device pointers, enqueued on `stream`.  Every output
 * pointer may be NULL (not wanted: not written); a NULL cotangent reads as zero; B == 0 returns 0.
 * No atomics: every output element is written by one thread that sums its contributions in a
 * fixed order, so two calls return the same bits.
 * ====================================================================== */

/* mpcqp_ltv_assemble_device / mpcqp_incr_assemble_device with the weights of this call: dQ, dQN
 * (nx*nx) and dR (nu*nu) are device arrays, dense row-major, shared by the batch, each NULL = the
 * layout's own.  dPx[nnzP] (may be NULL) receives ONE copy of P's stored values from those
 * weights in the pattern fixed at creation: a stored entry whose weight is now 0 stays as an
 * explicit zero, and a weight the pattern does not store (zero at creation) enters q only.
 * With dQ = dQN = dR = NULL the outputs are those of the plain entry point, bit for bit, and dPx
 * is mpcqp_*_layout_pattern's Px.  The weights pass through a scratch the layout owns: calls
 * with weights on one layout are to be ordered on one stream. */
int mpcqp_ltv_assemble_w_device(const mpcqp_ltv_layout *L, int64_t B, const double *dAd, const double *dBd,
                                const double *dgd, const double *dx0, const double *dXr, const double *dxlo,
                                const double *dxhi, const double *dQ, const double *dQN, const double *dR, double *dAx,
                                double *dq, double *dl, double *du, double *dPx, void *stream);
int mpcqp_incr_assemble_w_device(const mpcqp_incr_layout *L, int64_t B, const double *dAd, const double *dBd,
                                 const double *dgd, const double *dxt0, const double *dXr, const double *dQ,
                                 const double *dQN, const double *dR, double *dAx, double *dq, double *dl, double *du,
                                 double *dPx, void *stream);

/* The transpose of mpcqp_ltv_assemble_device / mpcqp_incr_assemble_device (nxa = nx for the LTV
 * layout, nx + nu for the incremental one).  Cotangents: gPx[b*nnzP], gAx[b*nnzA], gq[b*n],
 * gl[b*m], gu[b*m].  Of the forward call's inputs: Xr (read for gQ / gQN only), xlo / xhi (read
 * for gxlo / gxhi only), and dQ / dQN when the forward was *_assemble_w_device with them (NULL:
 * the layout's own).  Outputs, shaped as the forward's inputs:
 *   gAd[b,k,i,j] = gAx at the slot of that entry;  0 where maskA is 0;
 *   gBd[b,k,i,j] = the sum of gAx over its slots in CSC order -- one in the LTV layout, two in the
 *     incremental one (A~_k's upper-right block, then B~_k);  0 where maskB is 0;
 *   ggd[b,k,i]   = -(gl + gu)[(k+1) nxa + i];
 *   gx0[b,i]     = -(gl + gu)[i], i < nxa  (gxt0 of the incremental layout);
 *   gXr[b,j,k]   = -sum_{i < nx} W_k[i][j] gq[k nxa + i], i ascending, W_k what the forward
 *     multiplied with: Q (k < N) / QN (k = N) in the LTV layout, (Q C)' = Q' / QN' in the
 *     incremental one;
 *   gxlo / gxhi[b,k,i] = gl / gu[(N+1) nxa + k nxa + i] where -1e30 < xlo / xhi < 1e30, 0 where
 *     the forward clipped the bound (LTV layout only; MPCQP_EINVAL without the forward's xlo / xhi);
 *   gQ[b,i,j] = sum_{k < N} gPx[slot of stage k's Q[i][j]] - sum_{k < N} gq[k nxa + i] Xr[j,k]  (LTV),
 *     with gq[k nxa + j] Xr[i,k] in the second sum for the incremental layout (its q reads Q');
 *     gQN[b,i,j] the same over k = N alone;  gR[b,i,j] = sum_{k < N} gPx[slot of stage k's R[i][j]].
 *     Each sum runs over k ascending, the P part first.  These are the gradients WITH RESPECT TO
 *     THE STORED WEIGHTS, in the orientation of the Q, QN, R given to *_layout_create: P stores
 *     W[i][j] for i <= j where it was nonzero at creation, so only those entries have a P part
 *     (which, as mpcqp_adjoint_device's gPx, counts both symmetric positions); every other entry
 *     gets its q part alone.  Per instance: the caller sums over the batch for shared weights. */
int mpcqp_ltv_assemble_vjp_device(const mpcqp_ltv_layout *L, int64_t B, const double *dgPx, const double *dgAx,
                                  const double *dgq, const double *dgl, const double *dgu, const double *dXr,
                                  const double *dxlo, const double *dxhi, const double *dQ, const double *dQN,
                                  double *dgAd, double *dgBd, double *dggd, double *dgx0, double *dgXr, double *dgxlo,
                                  double *dgxhi, double *dgQ, double *dgQN, double *dgR, void *stream);
int mpcqp_incr_assemble_vjp_device(const mpcqp_incr_layout *L, int64_t B, const double *dgPx, const double *dgAx,
                                   const double *dgq, const double *dgl, const double *dgu, const double *dXr,
                                   const double *dQ, const double *dQN, double *dgAd, double *dgBd, double *dggd,
                                   double *dgxt0, double *dgXr, double *dgQ, double *dgQN, double *dgR, void *stream);

/* The transpose of mpcqp_affine_apply_device: with g the concatenation of the cotangents of the
 * three segments, g0[b*seglen0], g1[b*seglen1], g2[b*seglen2],
 *     gtheta[b*gtheta_stride + p] = sum over entries i and terms t with idx[i*T + t] == p of
 *                                   coef[i*T + t] * g[i]      (i ascending, then t;  p < nparam,
 * nparam = 1 + the largest idx given to mpcqp_affine_create; columns beyond are not written).
 * The regime selects only the base, which has no derivative: dregime is taken for symmetry with
 * the forward call and ignored. */
int mpcqp_affine_vjp_device(const mpcqp_affine *a, int64_t B, const double *dg0, const double *dg1, const double *dg2,
                            const int32_t *dregime, double *dgtheta, int32_t gtheta_stride, void *stream);

/* The VJP of mpcqp_kin_linearise_device per (vehicle, stage), from the closed form of
 * get_kinematics_model: x, u with the forward call's strides; cotangents gAd[(b*N + k)*16],
 * gBd[(b*N + k)*8], ggd[(b*N + k)*4]; outputs DENSE gx[(b*N + k)*4], gu[(b*N + k)*2] whatever the
 * strides (a forward with stage stride 0 -- one model for every stage -- leaves the sum over the
 * stages to the caller).  Only v, yaw and steer carry derivative; with c = cos, s = sin of yaw,
 * d = steer, wb = l_f + l_r, sec2 = 1 / cos^2 d, dsec2 = 2 sin d / cos^3 d:
 *   gx[2] = dt ((gAd13 c - gAd03 s) + (ggd0 s - ggd1 c) yaw + (gBd30 - ggd3 d) sec2 / wb)
 *   gx[3] = dt ((gAd12 c - gAd02 s) - v (gAd03 c + gAd13 s) + v (ggd0 (c yaw + s) + ggd1 (s yaw - c)))
 *   gu[0] = dt / wb (gAd32 sec2 + v (gBd30 dsec2 - ggd3 (sec2 + d dsec2)))
 * and gx[0] = gx[1] = gu[1] = 0 are written.  A NULL cotangent is zero; a NULL gx or gu is not
 * written.  The dynamic bicycle's linearisation has its own: mpcqp_linearise_vjp_device. */
int mpcqp_kin_linearise_vjp_device(const mpcqp_kin_vehicle *veh, int64_t B, int32_t N, const double *dx, int64_t x_sb,
                                   int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk, const double *dgAd,
                                   const double *dgBd, const double *dggd, double *dgx, double *dgu, int32_t device,
                                   void *stream);

/* The VJP of mpcqp_linearise_device (the dynamic bicycle: Pacejka tyres, the low-speed guard) per
 * (vehicle, stage): x, u with the forward call's strides (a stage stride of 0 included; the sum
 * over the stages is then the caller's); cotangents gAd[(b*N + k)*36], gBd[(b*N + k)*12],
 * ggd[(b*N + k)*6], each NULL = zero; outputs DENSE gx[(b*N + k)*6], gu[(b*N + k)*2], either NULL
 * = not written.  With (Ad, Bd, gd) = F(x, u) the forward AS IT COMPUTES,
 *   gx[j] = sum_il gAd_il dAd_il/dx_j + sum_il gBd_il dBd_il/dx_j + sum_i ggd_i dgd_i/dx_j,
 * and gu[j] alike in u_j, where
 *   Ad = I + dt Ac,  Bd = dt Bc,  gd = dt (f - Ac x~ - Bc u~)
 * at the guarded point (x~, u~), with get_dynamics_model's f, Ac and Bc.  That Ac is not
 * everywhere the derivative of that f (its dFx/dvx = -cda vx is the derivative of
 * -0.5 cda vx^2 sgn(vx) for vx > 0 only), so df/dx_j and Ac[:, j] in dgd/dx_j do not cancel and
 * both are formed; sgn(vx) has derivative 0.  The derivatives are exact ones of those formulas
 * (forward-mode dual numbers in yaw, vx, vy, r, steer, accel, contracted with the cotangents),
 * not difference quotients.
 *   X and Y never enter:                        gx[0] = gx[1] = 0 are written;
 *   |vx| < 0.5 (vx = 0 on the positive side):   the guard replaced vy, r and steer by 0:
 *                                               gx[4] = gx[5] = gu[0] = 0;
 *   |vx| < 0.3:                                 it replaced vx by +-0.3 as well: gx[3] = 0;
 * so below 0.3 only yaw and accel carry derivative, between 0.3 and 0.5 yaw, vx and accel, and
 * above 0.5 yaw, vx, vy, r, steer and accel (accel through Fx = m accel - ..., which enters Bc's
 * steer column and gd).  No atomics: each output element has one writer and identical calls give
 * identical bits.  MPCQP_EINVAL ("linearise_vjp: bad arguments") for a NULL veh, dx or du, B < 0
 * or N < 1, before any device call. */
int mpcqp_linearise_vjp_device(const mpcqp_vehicle *veh, int64_t B, int32_t N, const double *dx, int64_t x_sb,
                               int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk, const double *dgAd,
                               const double *dgBd, const double *dggd, double *dgx, double *dgu, int32_t device,
                               void *stream);

/* ======================================================================
 * Fleets: a batch of DIFFERENT vehicles.  Every entry point above that takes a
 * vehicle struct applies it to all B vehicles; its `_fleet` twin below takes a table of B
 * structs' constants instead and vehicle b uses entry b.
 * ====================================================================== */

/* veh is a HOST array of B structs.  Creation validates them and derives each vehicle's model
 * constants on the host with the formulas the uniform entry points use (the dynamic bicycle's
 * Iz, roll and drag terms and Pacejka coefficients; the kinematic bicycle has none derived), so
 * vehicle b of a fleet carries exactly the constants a uniform call with veh[b] passes.  It
 * makes no device call: the table is uploaded to `device` by the first device call that takes
 * the fleet.  MPCQP_EINVAL with a "fleet_create: ..." message for a NULL veh or out, B < 1, a
 * non-finite field, m, l_f, l_r or dt <= 0, width^2 + length^2 = 0, or a dt that is not the same
 * double in every entry (the reference search and the QP's horizon have one dt). */
typedef struct mpcqp_fleet mpcqp_fleet;         /* dynamic bicycle   */
typedef struct mpcqp_kin_fleet mpcqp_kin_fleet; /* kinematic bicycle */
int mpcqp_fleet_create(int64_t B, const mpcqp_vehicle *veh, int32_t device, mpcqp_fleet **out);
int mpcqp_kin_fleet_create(int64_t B, const mpcqp_kin_vehicle *veh, int32_t device, mpcqp_kin_fleet **out);
/* Host only: vehicle b's thirteen derived doubles, (m, l_f, l_r, Iz, dt, roh C_d A_f,
 * C_roll m 9.81, B_f, C_f, D_f, B_r, C_r, D_r). */
int mpcqp_fleet_constants(const mpcqp_fleet *f, int64_t b, double *out13);
void mpcqp_fleet_free(mpcqp_fleet *f);
void mpcqp_kin_fleet_free(mpcqp_kin_fleet *f);

/* The twelve twins: the signature of the entry point named without `_fleet`, the fleet in place of
 * the vehicle, and that entry point's semantics and argument checks; a B-vehicle call returns the
 * bits of the B uniform calls with veh[b] on vehicle b alone.  Added, as MPCQP_EINVAL before any
 * device call: a NULL fleet, a B that is not the fleet's size, a call on another device than the
 * fleet's (the `device` argument, or the layout's). */
int mpcqp_linearise_fleet_device(const mpcqp_fleet *f, int64_t B, int32_t N, const double *dx, int64_t x_sb,
                                 int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk, double *dAd, double *dBd,
                                 double *dgd, int32_t device, void *stream);
int mpcqp_linearise_vjp_fleet_device(const mpcqp_fleet *f, int64_t B, int32_t N, const double *dx, int64_t x_sb,
                                     int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk, const double *dgAd,
                                     const double *dgBd, const double *dggd, double *dgx, double *dgu, int32_t device,
                                     void *stream);
int mpcqp_incr_shift_fleet_device(const mpcqp_incr_layout *L, const mpcqp_fleet *f, int64_t B, const double *dsol,
                                  const double *dAd, const double *dBd, const double *dgd, double *dxt, double *dpred,
                                  double *dpdu, void *stream);
int mpcqp_incr_shift_vjp_fleet_device(const mpcqp_incr_layout *L, const mpcqp_fleet *f, int64_t B, const double *dsol,
                                      const double *dAd, const double *dBd, const double *dgd,
                                      const double *dxt_before, const double *dgxt, const double *dgpred,
                                      const double *dgpdu, double *dgsol, double *dgAd0, double *dgBd0, double *dggd0,
                                      double *dgxt_before, void *stream);
int mpcqp_kin_linearise_fleet_device(const mpcqp_kin_fleet *f, int64_t B, int32_t N, const double *dx, int64_t x_sb,
                                     int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk, double *dAd,
                                     double *dBd, double *dgd, int32_t device, void *stream);
int mpcqp_kin_linearise_vjp_fleet_device(const mpcqp_kin_fleet *f, int64_t B, int32_t N, const double *dx,
                                         int64_t x_sb, int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk,
                                         const double *dgAd, const double *dgBd, const double *dggd, double *dgx,
                                         double *dgu, int32_t device, void *stream);
int mpcqp_kin_shift_fleet_device(const mpcqp_incr_layout *L, const mpcqp_kin_fleet *f, int64_t B, const double *dsol,
                                 const double *dAd, const double *dBd, const double *dgd, const double *dXr,
                                 double *dxt, double *dpred, double *dpdu, int32_t *dfinish_cnt, int32_t *ddone,
                                 double *dtraj, int32_t traj_cap, int32_t *dtraj_len, void *stream);
int mpcqp_kin_shift_vjp_fleet_device(const mpcqp_incr_layout *L, const mpcqp_kin_fleet *f, int64_t B,
                                     const double *dsol, const double *dAd, const double *dBd, const double *dgd,
                                     const double *dxt_before, const int32_t *dmode, const double *dgxt,
                                     const double *dgpred, const double *dgpdu, double *dgsol, double *dgAd0,
                                     double *dgBd0, double *dggd0, double *dgxt_before, void *stream);
int mpcqp_kin_rollout_fleet_device(const mpcqp_kin_fleet *f, int64_t B, int32_t N, const double *dx0,
                                   const double *du0, double *dpred_x, double *dpred_u, int32_t device, void *stream);
int mpcqp_kin_ltv_shift_fleet_device(const mpcqp_ltv_layout *L, const mpcqp_kin_fleet *f, int64_t B,
                                     const double *dsol, const int32_t *dstatus, const double *dAd, const double *dBd,
                                     const double *dgd, double *dx, double *du, double *dpred_x, double *dpred_u,
                                     int32_t *dskipped, int32_t *dsteps_taken, double *dtraj, int32_t traj_cap,
                                     int32_t *dtraj_len, void *stream);
int mpcqp_kin_ltv_shift_vjp_fleet_device(const mpcqp_ltv_layout *L, const mpcqp_kin_fleet *f, int64_t B,
                                         const double *dsol, const double *dAd, const double *dBd,
                                         const double *dx_before, const int32_t *dmode, const double *dgx,
                                         const double *dgu, const double *dgpred_x, const double *dgpred_u,
                                         double *dgsol, double *dgAd0, double *dgBd0, double *dggd0,
                                         double *dgx_before, void *stream);
int mpcqp_lane_tail_fleet_device(const mpcqp_incr_layout *L, const mpcqp_kin_fleet *f, int64_t B, const double *dsol,
                                 const double *dAd, const double *dBd, const double *dgd, double *dxt, double *dpred,
                                 double *dpdu, int32_t nsw, const int32_t *switch_steps, const int32_t *paths_of,
                                 int32_t *dstep, int32_t *dpath_id, double *dtraj, int32_t traj_cap,
                                 int32_t *dtraj_len, void *stream);

/* ======================================================================
 * Gradients with respect to the vehicle parameters.  Fleet form only: the
 * cotangent has the table's shape, one row per vehicle; a uniform vehicle is a fleet of copies
 * whose rows the caller sums.  Coordinates are the ones the kernels read:
 *   dynamic bicycle    dgK (B, 13): (m, l_f, l_r, Iz, dt, cda, roll, B_f, C_f, D_f, B_r, C_r, D_r),
 *                      mpcqp_fleet_constants' order
 *   kinematic bicycle  dgK (B, 3):  (l_f, l_r, dt), the struct's
 * Each differentiates the forward as it computes, by the rules of mpcqp_linearise_vjp_device: the
 * low-speed guard first, an input it replaced is a constant, sgn(vx) has derivative 0, Ac as the
 * reference writes it; dt carries derivative through Ad = I + dt Ac, Bd = dt Bc, gd = dt (...) and
 * the Euler steps.  Every element of dgK is written (no accumulation into it).  A NULL cotangent
 * means zero.  MPCQP_EINVAL ("<name>: bad arguments") for a NULL fleet, point or dgK, B < 0, N < 1;
 * the fleet's own refusals (B, device) as its other entry points; all before any device call.
 * (B = 0, a no-op where a struct is taken, cannot be a fleet's size: it is that refusal.)
 * ====================================================================== */

/* The linearisations: x, u, dgAd, dgBd, dggd as mpcqp_linearise_vjp_device /
 * mpcqp_kin_linearise_vjp_device take them; dgK[b] is the sum over the N stages of vehicle b.
 * The sum is deterministic: one block holds 256 / N whole vehicles, every (vehicle, stage)
 * thread leaves its partial on chip, and one thread per output element adds them in stage order,
 * acc = 0, acc += partial[s] for s = 0 .. N-1; a repeated call returns the same bits.  That shape
 * needs N <= 256: a larger N returns MPCQP_EUNSUPPORTED before any device call. */
int mpcqp_linearise_pvjp_fleet_device(const mpcqp_fleet *f, int64_t B, int32_t N, const double *dx, int64_t x_sb,
                                      int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk, const double *dgAd,
                                      const double *dgBd, const double *dggd, double *dgK, int32_t device,
                                      void *stream);
int mpcqp_kin_linearise_pvjp_fleet_device(const mpcqp_kin_fleet *f, int64_t B, int32_t N, const double *dx,
                                          int64_t x_sb, int64_t x_sk, const double *du, int64_t u_sb, int64_t u_sk,
                                          const double *dgAd, const double *dgBd, const double *dggd, double *dgK,
                                          int32_t device, void *stream);
/* The terminal steps of the loop tails (the only place the constants enter a tail: its plant step
 * is affine in stage 0's Ad, Bd, gd): update_dynamics_model's guarded Euler step, x (6) u (2), and
 * update_kinematics_model, x (4) u (2), each read at a batch stride (x_sb, u_sb doubles between
 * vehicles) so that views into a taped solution can be passed.  dw (B, 6) / (B, 4) dense: the
 * cotangent of the new state.  dmode (B) or NULL: a vehicle whose mode is not 0 did not take the
 * step (the tails' stop and skip masks) and gets a zero row. */
int mpcqp_euler_step_pvjp_fleet_device(const mpcqp_fleet *f, int64_t B, const double *dx, int64_t x_sb,
                                       const double *du, int64_t u_sb, const double *dw, const int32_t *dmode,
                                       double *dgK, int32_t device, void *stream);
int mpcqp_kin_update_pvjp_fleet_device(const mpcqp_kin_fleet *f, int64_t B, const double *dx, int64_t x_sb,
                                       const double *du, int64_t u_sb, const double *dw, const int32_t *dmode,
                                       double *dgK, int32_t device, void *stream);
/* Host only, no device call: the chain from the thirteen constants back to the constructor
 * arguments, gveh = J' gk with J the Jacobian at *veh of the derivation mpcqp_fleet_create
 * applies, formed by running that derivation over dual numbers; gveh in the struct's field order
 * (m, l_f, l_r, width, length, C_d, A_f, C_roll, dt).  The kinematic struct derives nothing: its
 * chain is the identity. */
int mpcqp_vehicle_constants_vjp(const mpcqp_vehicle *veh, const double gk[13], double gveh[9]);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_H */
