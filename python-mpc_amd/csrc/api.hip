// api.hip -- C ABI of libmpcqp.so (declared in include/mpcqp.h).
//
// Host side of the drop-in boundary for `osqp.OSQP().setup()/update()/solve()`
// (vehicle_lateral_mpc_slack_increment.py:118-121,237,248,269;
// Control/MPC/mpc_dynamics.py:392-396).  The host only performs the symbolic
// analysis of the shared sparsity pattern (plan.cpp), memory management and
// kernel launches; every per-instance number is computed by the HIP kernels in
// kernels.hip.  There is no CPU fallback: without a HIP device every entry
// point that needs one returns MPCQP_EDEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mpcqp.h"
#include "kernels.h"
#include "plan.h"

using namespace mpcqp;

namespace {

thread_local std::string g_err;

// MPCQP_SETUP_TRACE=1 (diagnostic): the host-side stages of a setup call, in microseconds
// since the previous mark, on stderr
struct SetupTrace {
    bool on = false;
    std::chrono::steady_clock::time_point t;
    SetupTrace() {
        const char* e = getenv("MPCQP_SETUP_TRACE");
        on = e && e[0] == '1';
        t = std::chrono::steady_clock::now();
    }
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "mpcqp setup: %-22s %8.1f us\n", what,
                std::chrono::duration<double, std::micro>(now - t).count());
        t = now;
    }
};
SetupTrace& strace() {
    static thread_local SetupTrace tr;
    return tr;
}

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

}  // namespace

// shared with the other translation units of the library (the mpc_*.hip files)
int mpcqp::set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

namespace {

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(MPCQP_EDEVICE, "%s failed: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

struct Shard {
    int dev = 0;
    long b0 = 0, B = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // stream ordering of the calls on the handle: last_st is the stream of the last
    // call; a call on another stream records last_ev there and waits for it (enter)
    hipEvent_t last_ev = nullptr;
    hipStream_t last_st = nullptr;
    int* dplan = nullptr;
    void* dws = nullptr;    // one allocation for the whole workspace
    void* dio = nullptr;    // staging for the host-pointer API
    double *in_Px = nullptr, *in_Ax = nullptr, *in_q = nullptr, *in_l = nullptr, *in_u = nullptr;
    double *out_x = nullptr, *out_y = nullptr;
    // host-pointer API, small shards: pinned staging of everything a solve returns (x, y, the
    // info, the certificates, the statuses), filled by mpcqp_solve_batch with one
    // synchronisation; the info / certificate / polish getters then read it (mpcqp_handle::staged)
    char* hstage = nullptr;
    char* dstage = nullptr;  // the device side of hstage (launch_gather)
    char* hin = nullptr;  // ... and of update()'s q, l, u and the error flags it reads back
    size_t dws_bytes = 0, dplan_bytes = 0, hstage_bytes = 0, hin_bytes = 0, dstage_bytes = 0;  // (resource pool keys)
    unsigned long long dplan_tag = 0;  // Plan::uid of the device plan copy
    KParams kp{};
};

}  // namespace

struct mpcqp_handle {
    std::shared_ptr<const Plan> plan;  // shared with the plan cache (read-only)
    std::vector<int32_t> Pp, Pi, Ap, Ai;  // the user's pattern (a re-plan: replan_plain)
    mpcqp_settings set{};
    int n = 0, m = 0;
    long B = 0;
    std::vector<Shard> shards;
    bool timed = false;
    double last_ms = -1.0;
    bool collect = false;        // record hipEvent pairs around device solve launches
    bool collect_setup = false;  // ... and around device setup launches
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_setup, ev_solve;
    std::pair<hipEvent_t, hipEvent_t> last_pair{nullptr, nullptr};  // events of the last device solve
    bool staged = false;  // every shard's hstage holds the last mpcqp_solve_batch's results
    bool one_shot = false;    // mpcqp_set_one_shot: setup_solve_device persists no workspace state
    OneShot one_shot_loop = OneShot::dflt;  // MPCQP_ONE_SHOT_LOOP at creation (make_handle; one_shot_gl)
    bool state_gone = false;  // the last setup was one-shot: calls that read the workspace refuse
    bool solved = false;      // a solve has run on the current setup (mpcqp_adjoint_* needs its solution)
    bool has_setup = false;   // some setup has written the workspace (mpcqp_load_solution_device needs one)
};

namespace {

// calls that read what a setup leaves in the workspace (the scaled data, the iterates, the
// certificates) after a one-shot setup + solve, which left none of it
int need_state(const mpcqp_handle* h, const char* what) {
    if (h && h->state_gone)
        return fail(MPCQP_EINVAL, "%s: the last setup was one-shot (mpcqp_set_one_shot): the workspace keeps no "
                    "state; call a setup first", what);
    return 0;
}

bool env_is(const char* name, char c) {  // a one-character switch in the environment
    const char* e = getenv(name);
    return e && e[0] == c;
}

// the next region of a block: 256-byte aligned
size_t carve(size_t& off, size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    size_t o = off;
    off += bytes;
    return o;
}

// the plan-shape fields of KParams (what variant_fits reads)
void shape_params(const Plan& pl, KParams& k) {
    k.n = pl.n; k.m = pl.m; k.nb = pl.nb; k.npad = pl.npad; k.nnzP = pl.nnzP; k.nnzA = pl.nnzA; k.amax = pl.amax;
    k.bmax = pl.bmax; k.pmeet = (pl.nb - 1) / 2;
    k.ifok = pl.nb > 4 && pl.nb <= 64 && pl.amax <= 16 && pl.bmax <= 16 && pl.toff[k.pmeet] >= pl.amax &&
             pl.toff[k.pmeet] + pl.bmax <= kS;
    k.bsz01 = k.bsz23 = 1 << 20;
    if (pl.nb == 4) {
        k.bsz01 = std::max(pl.bsize[0], pl.bsize[1]);
        k.bsz23 = std::max(pl.bsize[2], pl.bsize[3]);
    }
    k.gk = pl.gather_k; k.pk = pl.p_k; k.ntgt = pl.ntgt; k.term_max = pl.term_max;
    k.gk1 = 0;
    for (int i = 128; i < pl.m; ++i) k.gk1 = std::max(k.gk1, pl.acsr_ptr[i + 1] - pl.acsr_ptr[i]);
    k.ne = pl.ne; k.ecnt = pl.ecnt; k.eterm_max = pl.eterm_max;
    k.gkr = pl.max_row_nnz; k.gkc = pl.max_col_nnz;
}

// ---- resource pool ----
// Device blocks, pinned host blocks and streams (with their three events) of freed handles,
// kept for the next handle of the same shape: the Control/MPC scripts set up a fresh osqp
// object every control step, and creating / destroying these costs most of a small setup
// (~0.4 ms).  A reused block is cleared exactly as a new one (alloc_shard's memset), a reused
// stream is idle (mpcqp_free synchronises it first).  Bounded: 256 MiB of device blocks,
// 64 MiB pinned, 8 streams; past that, resources are released as before.  The pool is never
// torn down (process exit reclaims it; no HIP call runs from a static destructor).
struct ResPool {
    struct Blk { int dev; size_t bytes; void* p; unsigned long long tag; };
    struct Str { int dev; hipStream_t st; hipEvent_t e0, e1, el; };
    std::mutex mu;
    std::vector<Blk> dev, pin;
    std::vector<Str> str;
    size_t dev_total = 0, pin_total = 0;
};
ResPool& respool() {
    static ResPool* p = new ResPool;
    return *p;
}
constexpr size_t kPoolDev = 256u << 20, kPoolPin = 64u << 20;
constexpr size_t kPoolStreams = 8;

// tag: what a block holds (a device plan's Plan::uid; 0 nothing reusable).  A block with the
// asked-for tag is preferred, and *hit says whether it was found (its contents are then the
// same as the caller would write).
hipError_t pool_malloc(int dev, size_t bytes, void** out, bool pinned, unsigned long long tag = 0,
                       bool* hit = nullptr) {
    ResPool& r = respool();
    if (hit) *hit = false;
    {
        std::lock_guard<std::mutex> lk(r.mu);
        auto& v = pinned ? r.pin : r.dev;
        size_t pick = v.size();
        for (size_t i = v.size(); i-- > 0;)
            if (v[i].dev == dev && v[i].bytes == bytes) {
                if (tag && v[i].tag == tag) { pick = i; break; }
                if (pick == v.size()) pick = i;
            }
        if (pick < v.size()) {
            *out = v[pick].p;
            if (hit) *hit = tag && v[pick].tag == tag;
            (pinned ? r.pin_total : r.dev_total) -= bytes;
            v.erase(v.begin() + pick);
            return hipSuccess;
        }
    }
    hipError_t e = pinned ? hipHostMalloc(out, bytes, hipHostMallocDefault) : hipMalloc(out, bytes);
    if (e == hipSuccess) return e;
    // out of memory: give the pooled blocks of this kind back (a caller that freed a handle to
    // make room must not fail where hipFree would have returned the memory) and try once more
    (void)hipGetLastError();
    std::vector<ResPool::Blk> rel;
    {
        std::lock_guard<std::mutex> lk(r.mu);
        auto& v = pinned ? r.pin : r.dev;
        for (size_t i = v.size(); i-- > 0;)
            if (pinned || v[i].dev == dev) {
                rel.push_back(v[i]);
                (pinned ? r.pin_total : r.dev_total) -= v[i].bytes;
                v.erase(v.begin() + i);
            }
    }
    if (rel.empty()) return e;
    for (auto& b : rel) {
        if (pinned) (void)hipHostFree(b.p);
        else (void)hipFree(b.p);
    }
    return pinned ? hipHostMalloc(out, bytes, hipHostMallocDefault) : hipMalloc(out, bytes);
}
void pool_free(int dev, size_t bytes, void* p, bool pinned, unsigned long long tag = 0) {
    if (!p) return;
    ResPool& r = respool();
    {
        std::lock_guard<std::mutex> lk(r.mu);
        size_t& tot = pinned ? r.pin_total : r.dev_total;
        if (tot + bytes <= (pinned ? kPoolPin : kPoolDev)) {
            (pinned ? r.pin : r.dev).push_back({dev, bytes, p, tag});
            tot += bytes;
            return;
        }
    }
    if (pinned) (void)hipHostFree(p);
    else (void)hipFree(p);
}
int pool_stream(Shard& s) {
    ResPool& r = respool();
    {
        std::lock_guard<std::mutex> lk(r.mu);
        for (size_t i = r.str.size(); i-- > 0;)
            if (r.str[i].dev == s.dev) {
                s.stream = r.str[i].st; s.ev0 = r.str[i].e0; s.ev1 = r.str[i].e1; s.last_ev = r.str[i].el;
                r.str.erase(r.str.begin() + i);
                return 0;
            }
    }
    HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&s.ev0));
    HIPCHK(hipEventCreate(&s.ev1));
    HIPCHK(hipEventCreateWithFlags(&s.last_ev, hipEventDisableTiming));
    return 0;
}
void pool_stream_release(Shard& s) {
    if (!s.stream) return;
    ResPool& r = respool();
    {
        std::lock_guard<std::mutex> lk(r.mu);
        if (r.str.size() < kPoolStreams && s.ev0 && s.ev1 && s.last_ev) {
            r.str.push_back({s.dev, s.stream, s.ev0, s.ev1, s.last_ev});
            return;
        }
    }
    if (s.ev0) (void)hipEventDestroy(s.ev0);
    if (s.ev1) (void)hipEventDestroy(s.ev1);
    if (s.last_ev) (void)hipEventDestroy(s.last_ev);
    (void)hipStreamDestroy(s.stream);
}

int upload_plan(const Plan& pl, Shard& s) {
    KParams& k = s.kp;
    struct Part { const std::vector<int>* v; const int** dst; };  // a plan array and its device pointer
    const Part parts[] = {
        {&pl.pad_var, &k.pad_var}, {&pl.acsc_ptr, &k.acsc_ptr}, {&pl.acsc_row, &k.acsc_row}, {&pl.acsc_v, &k.acsc_v},
        {&pl.acsr_ptr, &k.acsr_ptr}, {&pl.acsr_col, &k.acsr_col}, {&pl.acsr_v, &k.acsr_v},
        {&pl.psym_ptr, &k.psym_ptr}, {&pl.psym_col, &k.psym_col}, {&pl.psym_v, &k.psym_v},
        {&pl.p_r, &k.p_r}, {&pl.p_c, &k.p_c}, {&pl.a_r, &k.a_r}, {&pl.a_c, &k.a_c},
        {&pl.asm_blk_ptr, &k.asm_blk_ptr}, {&pl.asm_tgt, &k.asm_tgt}, {&pl.tterm, &k.tterm},
        {&pl.acsr_pos, &k.acsr_pos}, {&pl.gcol, &k.gcol}, {&pl.grow, &k.grow}, {&pl.gpsym, &k.gpsym},
        {&pl.toff, &k.toff}, {&pl.bsize, &k.bsize}, {&pl.tcnt, &k.tcnt}, {&pl.eown, &k.eown},
        {&pl.etterm, &k.etterm}, {&pl.wide_cg, &k.wcg}, {&pl.wide_pg, &k.wpg}, {&pl.wide_rg, &k.wrg},
        {&pl.wide_as, &k.was}, {&pl.wide_ps, &k.wps}, {&pl.csc_pos, &k.csc_pos}};
    size_t total = 0;
    for (auto& p : parts) total += p.v->size() + 1;  // never allocate zero-length parts
    s.dplan_bytes = total * sizeof(int);
    s.dplan_tag = pl.uid;
    bool have = false;  // a pooled copy of this very plan (a fresh handle of the same pattern)
    HIPCHK(pool_malloc(s.dev, s.dplan_bytes, (void**)&s.dplan, false, pl.uid, &have));
    if (!have) {  // (the flat image is built only when it is uploaded)
        std::vector<int> flat;
        flat.reserve(total);
        for (auto& p : parts) {
            flat.insert(flat.end(), p.v->begin(), p.v->end());
            flat.push_back(0);
        }
        HIPCHK(hipMemcpy(s.dplan, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    size_t off = 0;
    for (auto& p : parts) {
        *p.dst = s.dplan + off;
        off += p.v->size() + 1;
    }
    return 0;
}

// ---- the workspace (Shard::dws): one listing ----
// Every region in carve order, each on a 256-byte boundary: the KParams / Shard pointer it is
// carved into, its element size and count, and what a re-plan does with it.  workspace_bytes,
// alloc_shard's carve and replan_plain's copies are passes over this listing.
enum class Carry {
    copy,    // moved verbatim
    by_var,  // per column, padded order: old var_pad -> new var_pad, the padding set to Region::pad
    by_csc,  // the scaled A values: old csc_pos -> new csc_pos
    drop     // rebuilt by the next solve (the factor), restarted (the dispatch order) or the block's own
};
struct Region {
    void* slot;  // the pointer member's address
    size_t esz, count;
    Carry carry;
    double pad;
    bool carved;  // false: counted in the size, but the pointer stays null and the carve skips it
};
void* region_ptr(const Region& r) {
    void* p;
    memcpy(&p, r.slot, sizeof p);
    return p;
}

std::vector<Region> workspace_regions(const Plan& pl, long B, bool with_io, Shard& s) {
    KParams& k = s.kp;
    const size_t b = B, n = pl.n, m = pl.m, np = pl.npad, fac = (size_t)pl.nb * kS * kS;
    const size_t kd = dense_rows_doubles(pl.nb, pl.ne);  // (zero in the production build)
    std::vector<Region> r;
    r.reserve(48);
    auto add = [&](auto*& p, size_t count, Carry c, double pad = 0.0, bool carved = true) {
        r.push_back({(void*)&p, sizeof(*p), count, c, pad, carved});
    };
    const Carry cp = Carry::copy, no = Carry::drop;
    add(k.Px, b * pl.nnzP, cp); add(k.Ax, b * pl.nnzA, Carry::by_csc);
    add(k.q, b * np, Carry::by_var, 0.0); add(k.D, b * np, Carry::by_var, 1.0);
    add(k.l, b * m, cp); add(k.u, b * m, cp); add(k.E, b * m, cp);
    add(k.x, b * np, Carry::by_var, 0.0); add(k.z, b * m, cp); add(k.y, b * m, cp);
    add(k.scal, b * 4, cp);
    add(k.F, b * fac, no); add(k.H, b * fac, no); add(k.Si, b * fac, no);
    add(k.Kd, b * kd, no, 0.0, kd != 0);
    add(k.dyc, b * m, cp); add(k.dxc, b * n, cp);  // certificates
    add(k.obj, b, cp); add(k.pri, b, cp); add(k.dua, b, cp); add(k.rho_est, b, cp);
    add(k.ct, b * m, cp);
    // err right before status: check_setup reads both in one copy, from err to the end of status
    add(k.err, b, cp); add(k.status, b, cp);
    add(k.iter, b, cp); add(k.rho_upd, b, cp); add(k.pstat, b, cp);
    add(k.ffresh, b, no);
    add(k.order, b, no); add(k.pred, b, no);  // (alloc_shard fills order with the identity)
    add(k.done, 1, no);   // (fused order epilogue; alloc_shard keeps it for some variants only)
    add(k.queue, 2, no);  // (k_solve_b's persistent form)
    add(k.prof, b * kProfSlots, no, 0.0, env_is("MPCQP_PHASE_PROF", '1'));  // (always counted)
    add(k.self, 1, no);
    if (with_io) {  // the host-pointer API's device inputs and outputs; the five inputs in one run
        add(s.in_Px, b * pl.nnzP, cp); add(s.in_Ax, b * pl.nnzA, cp);
        add(s.in_q, b * n, cp); add(s.in_l, b * m, cp); add(s.in_u, b * m, cp);
        add(s.out_x, b * n, cp); add(s.out_y, b * m, cp);
    }
    return r;
}

size_t workspace_bytes(const Plan& pl, long B, bool with_io) {
    Shard none;
    size_t off = 0;
    for (const Region& r : workspace_regions(pl, B, with_io, none)) carve(off, r.esz * r.count);
    return off + 256;
}

// The settings a running handle may change (mpcqp_update_settings), as (KParams, mpcqp_settings)
// member pairs.  rho_interval is not among them: OSQP resolves the automatic interval in
// osqp_setup, so check_termination set later does not move it.
template <class F>
void each_mutable_setting(F&& f) {
    using K = KParams;
    using S = mpcqp_settings;
    f(&K::alpha, &S::alpha); f(&K::eps_abs, &S::eps_abs); f(&K::eps_rel, &S::eps_rel);
    f(&K::eps_pinf, &S::eps_prim_inf); f(&K::eps_dinf, &S::eps_dual_inf); f(&K::rho0, &S::rho);
    f(&K::max_iter, &S::max_iter); f(&K::check_term, &S::check_termination); f(&K::warm_start, &S::warm_start);
    f(&K::scaled_term, &S::scaled_termination); f(&K::polish, &S::polish);
    f(&K::refine_iter, &S::polish_refine_iter); f(&K::delta, &S::delta);
}
void apply_settings(KParams& k, const mpcqp_settings& st) {
    each_mutable_setting([&](auto kf, auto sf) { k.*kf = st.*sf; });
}
void carry_settings(KParams& to, const KParams& from) {  // (replan_plain)
    each_mutable_setting([&](auto kf, auto) { to.*kf = from.*kf; });
}

// The solve variant of a plan's shape: the production choice (-1: no instantiation fits), the
// MPCQP_VARIANT override (diagnostic: A/B timing) and the variant's mode.
int pick_variant(KParams& k) {
    k.variant = solve_variant(k);
    if (const char* ev = getenv("MPCQP_VARIANT"); ev && *ev) {
        const int v = atoi(ev);
        if (!variant_fits(k, v)) return fail(MPCQP_EUNSUPPORTED, "MPCQP_VARIANT=%d does not fit this plan", v);
        k.variant = v;
    }
    k.mode = k.variant >= 0 ? solve_mode(k.variant) : 0;
    return 0;
}

// what mpcqp_get_plan_info and mpcqp_plan_preview report of a plan and its variant (k: shape,
// variant and mode filled; null: no shard)
void fill_plan_info(mpcqp_plan_info* info, int n, int m, const Plan& pl, const KParams* k) {
    const bool have = k && k->variant >= 0;
    info->n = n; info->m = m; info->nb = pl.nb; info->block = kS; info->npad = pl.npad;
    info->max_level = pl.max_level;
    info->lds_bytes_solve = have ? (int64_t)lds_kernel_bytes(*k) : 0;
    info->bytes_per_instance = (int64_t)workspace_bytes(pl, 1, false);
    info->amax = pl.amax; info->gather_k = pl.gather_k;
    info->variant = k ? k->variant : -1;
    info->threads_per_qp = have ? solve_threads(k->variant) : 0;
    info->n_eliminated = pl.ne; info->plan_choice = pl.choice;
}

// sync: wait for the zeroing, the identity order and the parameter block before returning (the
// device API's callers may use the workspace from any stream; the host batch setup queues all
// its work on the shard's stream behind them and waits once, in check_setup)
int alloc_shard(mpcqp_handle* h, Shard& s, bool with_io, bool sync = true) {
    const Plan& pl = *h->plan;
    HIPCHK(hipSetDevice(s.dev));
    if (int e = pool_stream(s)) return e;
    strace().mark("stream");
    if (int e = upload_plan(pl, s)) return e;
    strace().mark("plan upload");
    const long B = s.B;
    size_t total = workspace_bytes(pl, B, with_io);
    hipError_t e = pool_malloc(s.dev, total, &s.dws, false);
    if (e == hipSuccess) s.dws_bytes = total;
    if (e != hipSuccess)
        return fail(MPCQP_ENOMEM, "hipMalloc(%zu bytes) failed: %s", total, hipGetErrorString(e));
    strace().mark("workspace alloc");
    HIPCHK(hipMemsetAsync(s.dws, 0, total, s.stream));
    strace().mark("workspace memset");
    KParams& k = s.kp;
    size_t off = 0;
    for (const Region& r : workspace_regions(pl, B, with_io, s)) {
        void* p = r.carved ? (char*)s.dws + carve(off, r.esz * r.count) : nullptr;
        memcpy(r.slot, &p, sizeof p);
    }
    if (off > total)
        return fail(MPCQP_EDEVICE, "workspace carve ends at %zu bytes, past the %zu bytes allocated", off, total);
    k.reuse = !env_is("MPCQP_FACTOR_REUSE", '0');
    k.apart = !env_is("MPCQP_MIDDLE_APART", '0');
    k.lchain = !env_is("MPCQP_LDS_CHAIN", '0');
    {  // dispatch order (kernels.hip::k_order), identity until the first solve; pred, done and
       // queue are zero from the memset above
        HIPCHK(launch_iota(const_cast<int*>(k.order), B, s.stream));
        const char* od = getenv("MPCQP_ORDER_DECAY");
        k.odecay = od ? std::max(0, std::min(8, atoi(od))) : 7;  // (tools/pred_sim.py, profiles/r6/dispatch.txt)
        strace().mark("order upload");
        if (const char* ev = getenv("MPCQP_DISPATCH"); ev && !strcmp(ev, "identity")) k.order = nullptr;  // A/B
    }
    k.qpersist = !env_is("MPCQP_PERSIST", '0');
    k.persist = 0;
    k.qn = 0;
    shape_params(pl, k);
    const mpcqp_settings& st = h->set;
    apply_settings(k, st);  // ... and the ones fixed at setup:
    k.sigma = st.sigma; k.rho_tol = st.adaptive_rho_tolerance; k.scaling = st.scaling; k.adaptive_rho = st.adaptive_rho;
    int interval = st.adaptive_rho_interval;
    if (st.adaptive_rho && interval == 0) interval = st.check_termination ? 4 * st.check_termination : 100;
    k.rho_interval = interval;
    if (solve_variant(k) < 0)
        return fail(MPCQP_EUNSUPPORTED, "problem shape outside the solve kernel's instantiations (n=%d m=%d)", pl.n, pl.m);
    if (int e = pick_variant(k)) return e;
    // some variants' kernels sort the next dispatch order in their last workgroup (MPCQP_ORDER_KERNEL=1: k_order)
    if (!(variant_of(k.variant)->order && k.order && !env_is("MPCQP_ORDER_KERNEL", '1'))) k.done = nullptr;
    {  // resident solve workgroups: below this batch size the dispatch order is moot
        int ncu = 0;
        HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, s.dev));
        const int occ = solve_blocks_per_cu(k);
        if (occ < 0) return fail(MPCQP_EDEVICE, "occupancy query for solve variant %d failed", k.variant);
        k.slots = (long)ncu * occ;
    }
    strace().mark("variant + occupancy");
    // the zeroing, the identity order and the parameter block in stream order, one wait for
    // all three (callers then use the workspace from any stream or from the host)
    HIPCHK(hipMemcpyAsync((void*)k.self, &k, sizeof(KParams), hipMemcpyHostToDevice, s.stream));
    if (sync) HIPCHK(hipStreamSynchronize(s.stream));
    strace().mark("params upload");
    if (size_t lds = lds_kernel_bytes(k); lds > 160 * 1024)
        return fail(MPCQP_EUNSUPPORTED, "problem needs %zu bytes of LDS per instance (> 160 KiB)", lds);
    return 0;
}

// The plan of a handle: with the degree <= 1 vertices of K eliminated (plan.h) when the
// four-wave kernel then runs the reduced system -- the slack layouts (SURVEY.md §8
// configs 1, 3, 4: 230 variables, 8 blocks -> 125 in 4) -- else the plain plan.  Polish
// factors the full system (factorize<POL>), so it keeps the plain plan; MPCQP_ELIM=0 (A/B)
// and an MPCQP_VARIANT override other than 17 do too.
// The plan's choice and, when an eliminated plan is rejected, why (Plan::choice /
// choice_note; MPCQP_PLAN_LOG=1 prints it): a regression in the level ordering or the
// greedy packing (e.g. amax > 8) then shows up in plan_info instead of as a quiet 2x
// slowdown on the plain plan.
std::string w4_misfit(const KParams& k) {
    char buf[256];
    const bool el = k.ne > 0;
    std::string r;
    auto need = [&](bool ok, const char* what, long have, long lim) {
        if (ok) return;
        snprintf(buf, sizeof buf, "%s%s = %ld > %ld", r.empty() ? "" : ", ", what, have, lim);
        r += buf;
    };
    if (k.nb != 4) {
        snprintf(buf, sizeof buf, "nb = %d (needs 4)", k.nb);
        r += buf;
    }
    need(k.amax <= 8, "amax", k.amax, 8);
    need(k.gkr <= 6, "longest A row", k.gkr, 6);
    need(k.gkc <= (el ? 8 : 6), "longest A column", k.gkc, el ? 8 : 6);
    need(k.pk <= 4, "longest P column", k.pk, 4);
    need(k.m <= 256, "m", k.m, 256);
    need(k.npad <= (el ? 256 : 128), "npad", k.npad, el ? 256 : 128);
    need(k.nnzA <= (el ? 768 : 512), "nnzA", k.nnzA, el ? 768 : 512);
    need(k.nnzP <= 256, "nnzP", k.nnzP, 256);
    if (el) need(k.ecnt <= 2, "A nonzeros of an eliminated column", k.ecnt, 2);
    if (el) need(k.ne <= 128, "eliminated columns", k.ne, 128);
    KParams q2 = k;
    q2.mode = 2;
    need(lds_w2_bytes(q2) <= 80 * 1024, "LDS bytes", (long)lds_w2_bytes(q2), 80 * 1024);
    return r.empty() ? "does not fit variant 17" : r;
}

unsigned long long next_plan_uid() {
    static std::atomic<unsigned long long> c{0};
    return ++c;
}

std::string choose_plan(int32_t n, int32_t m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                        const int32_t* Ai, const mpcqp_settings& st, Plan& pl) {
    const char* ev = getenv("MPCQP_ELIM");
    const char* vv = getenv("MPCQP_VARIANT");
    int choice = 0;
    std::string note;
    if (!st.polish && !(ev && ev[0] == '0') && !(vv && *vv && atoi(vv) != 17)) {
        std::string err = build_plan(n, m, Pp, Pi, Ap, Ai, pl, true);
        if (err.empty() && pl.ne > 0) {  // (nothing eliminated: the plain plan, level-merged blocks)
            KParams k{};
            shape_params(pl, k);
            k.mode = 2;
            if (variant_fits(k, 17)) {
                pl.choice = 1;
                pl.uid = next_plan_uid();
                return err;
            }
            choice = 2;
            note = "eliminated plan (" + std::to_string(pl.ne) + " columns, " + std::to_string(pl.nb) +
                   " blocks) rejected: " + w4_misfit(k);
        } else {
            choice = err.empty() ? 3 : 2;
            if (!err.empty()) note = "eliminated plan failed: " + err;
        }
    }
    std::string err = build_plan(n, m, Pp, Pi, Ap, Ai, pl, false, true);  // (balanced four-block merge: plan.cpp)
    pl.uid = next_plan_uid();
    pl.choice = choice;
    pl.choice_note = note;
    if (const char* lg = getenv("MPCQP_PLAN_LOG"); lg && lg[0] == '1' && !note.empty())
        fprintf(stderr, "mpcqp: %s; using the plain plan\n", note.c_str());
    return err;
}

// Plans by sparsity pattern: the Control/MPC scripts set up a fresh osqp object, with the same
// pattern, every control step (mpc_kinematics.py:194-198), and planning is most of a small
// setup's host time (~0.8 ms at N = 20).  A few recent plans are kept; a hit compares the whole
// pattern, the polish flag and the plan-choice overrides, so it returns exactly the plan
// choose_plan would build.
struct PlanKey {
    int32_t n = 0, m = 0;
    bool polish = false;
    std::string env;
    std::vector<int32_t> pat;
    bool operator==(const PlanKey& o) const {
        return n == o.n && m == o.m && polish == o.polish && env == o.env && pat == o.pat;
    }
};
std::mutex g_plan_mu;
std::vector<std::pair<PlanKey, std::shared_ptr<const Plan>>> g_plans;  // most recently used last
constexpr size_t kPlanCache = 8;

std::string cached_plan(int32_t n, int32_t m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                        const int32_t* Ai, const mpcqp_settings& st, std::shared_ptr<const Plan>& out) {
    auto fresh = [&]() {
        auto pl = std::make_shared<Plan>();
        std::string err = choose_plan(n, m, Pp, Pi, Ap, Ai, st, *pl);
        out = pl;
        return err;
    };
    if (n <= 0 || m < 0 || Pp[n] < 0 || Ap[n] < 0) return fresh();
    PlanKey k;
    k.n = n;
    k.m = m;
    k.polish = st.polish != 0;
    const char* ev = getenv("MPCQP_ELIM");
    const char* vv = getenv("MPCQP_VARIANT");
    k.env = std::string(ev ? ev : "") + "|" + (vv ? vv : "");
    k.pat.reserve(2 * ((size_t)n + 1) + (size_t)Pp[n] + (size_t)Ap[n]);
    k.pat.insert(k.pat.end(), Pp, Pp + n + 1);
    k.pat.insert(k.pat.end(), Pi, Pi + Pp[n]);
    k.pat.insert(k.pat.end(), Ap, Ap + n + 1);
    k.pat.insert(k.pat.end(), Ai, Ai + Ap[n]);
    {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        for (size_t i = g_plans.size(); i-- > 0;)
            if (g_plans[i].first == k) {
                out = g_plans[i].second;  // shared, not copied (a cfg-5 plan copy took ~35 us)
                std::rotate(g_plans.begin() + i, g_plans.begin() + i + 1, g_plans.end());
                return std::string();
            }
    }
    std::string err = fresh();
    if (err.empty()) {
        std::lock_guard<std::mutex> lk(g_plan_mu);
        g_plans.emplace_back(std::move(k), out);
        if (g_plans.size() > kPlanCache) g_plans.erase(g_plans.begin());
    }
    return err;
}

int validate_settings(const mpcqp_settings& s) {
    if (!(s.rho > 0) || !(s.sigma > 0) || s.max_iter <= 0 || s.eps_abs < 0 || s.eps_rel < 0 ||
        (s.eps_abs == 0 && s.eps_rel == 0) || !(s.eps_prim_inf > 0) || !(s.eps_dual_inf > 0) ||
        !(s.alpha > 0 && s.alpha < 2) || s.scaling < 0 || s.check_termination < 0 ||
        s.adaptive_rho_interval < 0 || !(s.adaptive_rho_tolerance >= 1))
        return fail(MPCQP_EINVAL, "invalid settings");
    if (s.polish && (!(s.delta > 0) || s.polish_refine_iter < 0)) return fail(MPCQP_EINVAL, "invalid polish settings");
    return 0;
}

int make_handle(int32_t n, int32_t m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                const int32_t* Ai, int64_t B, const mpcqp_settings* settings, std::vector<int> devs,
                bool with_io, mpcqp_handle** out) {
    if (!out) return fail(MPCQP_EINVAL, "out is NULL");
    *out = nullptr;
    if (B <= 0) return fail(MPCQP_EINVAL, "batch must be positive");
    if (!Pp || !Pi || !Ap || !Ai) return fail(MPCQP_EINVAL, "NULL pattern array");
    auto h = std::make_unique<mpcqp_handle>();
    if (settings) h->set = *settings;
    else mpcqp_default_settings(&h->set);
    if (int e = validate_settings(h->set)) return e;
    if (const char* ev = getenv("MPCQP_ONE_SHOT_LOOP")) {  // (before any device call; an unknown name is refused)
        constexpr struct { const char* name; OneShot loop; } names[] = {
            {"", OneShot::dflt}, {"lds", OneShot::lds}, {"wave", OneShot::wave}, {"roles", OneShot::roles}};
        h->one_shot_loop = OneShot::off;
        for (const auto& e : names)
            if (!strcmp(ev, e.name)) h->one_shot_loop = e.loop;
        if (h->one_shot_loop == OneShot::off)
            return fail(MPCQP_EINVAL, "MPCQP_ONE_SHOT_LOOP=%s: not one of lds, wave, roles (or empty: the default)", ev);
    }
    strace().mark("(enter)");
    std::string err = cached_plan(n, m, Pp, Pi, Ap, Ai, h->set, h->plan);
    strace().mark("plan");
    if (!err.empty()) {
        bool unsup = err.rfind("unsupported", 0) == 0;
        return fail(unsup ? MPCQP_EUNSUPPORTED : MPCQP_EINVAL, "%s", err.c_str());
    }
    h->n = n; h->m = m; h->B = B;
    h->Pp.assign(Pp, Pp + n + 1); h->Pi.assign(Pi, Pi + Pp[n]);
    h->Ap.assign(Ap, Ap + n + 1); h->Ai.assign(Ai, Ai + Ap[n]);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MPCQP_EDEVICE, "no HIP device available (the solver has no CPU fallback)");
    for (int d : devs)
        if (d < 0 || d >= ndev) return fail(MPCQP_EDEVICE, "device %d not present (%d devices)", d, ndev);
    const long nd = (long)devs.size();
    for (long i = 0; i < nd; ++i) {
        Shard s;
        s.dev = devs[i];  // devs may repeat a device (MPCQP_SPLIT): several shards on it, one stream each
        s.b0 = B * i / nd;
        s.B = B * (i + 1) / nd - s.b0;
        if (s.B <= 0) continue;
        h->shards.push_back(s);
    }
    for (auto& s : h->shards)
        if (int e = alloc_shard(h.get(), s, with_io, !with_io)) { mpcqp_free(h.release()); return e; }
    *out = h.release();
    return 0;
}

int check_bounds_host(const mpcqp_handle* h, const double* l, const double* u, long B) {
    if (!l || !u) return 0;
    const long m = h->m;
    for (long i = 0; i < B * m; ++i) {
        double li = std::max(l[i], -1e30), ui = std::min(u[i], 1e30);
        if (!(li <= ui))
            return fail(MPCQP_EINVAL, "instance %ld row %ld: lower bound must be lower than or equal to upper bound",
                        i / m, i % m);
    }
    return 0;
}

// waits for the handle's own streams and for the last call's work wherever it was
// enqueued (a caller stream of the *_device entry points: last_ev)
int sync_all(mpcqp_handle* h) {
    for (auto& s : h->shards) {
        HIPCHK(hipSetDevice(s.dev));
        HIPCHK(hipStreamSynchronize(s.stream));
        if (s.last_st) HIPCHK(hipEventSynchronize(s.last_ev));
    }
    return 0;
}

// Every call enqueues on one stream; work of the previous call on the handle that went
// to another stream is waited for first.  The handle's workspace -- including the
// dispatch order each solve rewrites for the next (kernels.hip::k_order) -- is then
// never read by one stream while another writes it, whatever streams the caller uses.
// stream_leave records last_ev on a caller's stream once the call's work is enqueued, so
// stream_enter never touches a stream of an earlier call (which the caller may have
// destroyed since): on a change of stream it only makes the new stream wait for last_ev.
// The handle's own stream is never destroyed before the handle, so a call on it records
// nothing: last_ev is recorded there only when the next call moves to another stream
// (a single-stream caller's queue holds kernels only -- no event packet between them).
int stream_enter(Shard& s, hipStream_t st) {
    if (s.last_st && s.last_st != st) {
        if (s.last_st == s.stream) HIPCHK(hipEventRecord(s.last_ev, s.stream));
        HIPCHK(hipStreamWaitEvent(st, s.last_ev, 0));
    }
    return 0;
}
int stream_leave(Shard& s, hipStream_t st) {
    if (st != s.stream) HIPCHK(hipEventRecord(s.last_ev, st));
    s.last_st = st;
    return 0;
}

// One call's work on one shard: body enqueues on st between stream_enter and stream_leave.
// stream_leave runs on every return path -- work may be queued on st before a HIP call fails,
// and the next call on another stream must still wait for it.  Inlined: no allocation, no lock.
template <class F>
int on_stream(Shard& s, hipStream_t st, F&& body) {
    HIPCHK(hipSetDevice(s.dev));
    if (int e = stream_enter(s, st)) return e;
    if (const int rc = body()) {
        const std::string why = g_err;  // body's error is the one reported
        (void)stream_leave(s, st);
        g_err = why;
        return rc;
    }
    return stream_leave(s, st);
}

// the first instance a setup / update kernel flagged (KParams::err), and the first one the
// factor-only solve found non-convex
int first_flagged(const int* err, long B, long b0) {
    for (long i = 0; i < B; ++i)
        if (err[i]) return fail(MPCQP_EINVAL, "instance %ld: invalid data (l > u or NaN bounds)", b0 + i);
    return 0;
}
int first_nonconvex(const int* status, long B, long b0) {
    for (long i = 0; i < B; ++i)
        if (status[i] == MPCQP_NON_CVX_)
            return fail(MPCQP_ENONCVX, "instance %ld: P is not convex (the KKT matrix is not quasi-definite)", b0 + i);
    return 0;
}
int shard_err_flags(Shard& s) {  // (synchronous: a shard past kStageMax, or outside the staged calls)
    std::vector<int> err(s.B);
    HIPCHK(hipSetDevice(s.dev));
    HIPCHK(hipMemcpy(err.data(), s.kp.err, sizeof(int) * s.B, hipMemcpyDeviceToHost));
    return first_flagged(err.data(), s.B, s.b0);
}
int check_err_flags(mpcqp_handle* h) {
    for (auto& s : h->shards)
        if (int e = shard_err_flags(s)) return e;
    return 0;
}

// ---- staging of the host-pointer API ----
// A call's arrays as segments.  A small shard packs them into a pinned block (at Seg::off) and
// moves them with one copy where the device side has the same layout (mirror), asynchronously
// and with one synchronisation per call; a shard past kStageMax bytes copies each array
// straight from / into the caller's memory as before (the large throughput batches, where the
// copies dominate).
constexpr size_t kStageMax = 16u << 20;
enum class Dir { up, down };
struct Seg {
    void* host;  // the caller's array, all instances (null: not given)
    void* dev;   // the shard's device array (down, null: zeros)
    long per;    // elements per instance
    int sz;      // element size
    Dir dir;
    size_t off;  // in the pinned block
};
size_t seg_bytes(const Seg& g, long Bs) { return (size_t)Bs * g.per * g.sz; }
char* seg_host(const Seg& g, long b0) { return (char*)g.host + (size_t)b0 * g.per * g.sz; }

// hb: the pinned block, null for direct copies; mirror: the device block laid out as hb, null
// when the device arrays lie elsewhere (then one copy per segment, out of hb)
int stage_up(Shard& s, const Seg* sg, size_t nseg, char* hb, void* mirror) {
    size_t end = 0;
    for (const Seg* g = sg; g != sg + nseg; ++g) {
        if (g->dir != Dir::up || !g->host) continue;
        const char* src = seg_host(*g, s.b0);
        const size_t by = seg_bytes(*g, s.B);
        if (hb) {
            memcpy(hb + g->off, src, by);
            src = hb + g->off;
            end = g->off + by;
        }
        if (!hb || !mirror) HIPCHK(hipMemcpyAsync(g->dev, src, by, hipMemcpyHostToDevice, s.stream));
    }
    if (hb && mirror) HIPCHK(hipMemcpyAsync(mirror, hb, end, hipMemcpyHostToDevice, s.stream));
    return 0;
}
int stage_down(Shard& s, const Seg* sg, size_t nseg, char* hb, const void* mirror, size_t bytes) {
    if (hb) {
        HIPCHK(hipMemcpyAsync(hb, mirror, bytes, hipMemcpyDeviceToHost, s.stream));
        return 0;
    }
    for (const Seg* g = sg; g != sg + nseg; ++g)
        if (g->dir == Dir::down && g->host)
            HIPCHK(hipMemcpyAsync(seg_host(*g, s.b0), g->dev, seg_bytes(*g, s.B), hipMemcpyDeviceToHost, s.stream));
    return 0;
}
void stage_unpack(const Shard& s, const Seg* sg, size_t nseg, const char* hb) {  // after the synchronisation
    for (const Seg* g = sg; g != sg + nseg; ++g)
        if (g->dir == Dir::down && g->host) memcpy(seg_host(*g, s.b0), hb + g->off, seg_bytes(*g, s.B));
}

// Shard::hin, the persistent pinned input block, serves three calls; whichever comes first
// allocates it for all of them:
//   mpcqp_setup_batch   the five inputs, laid out as in the workspace (input_span)
//   check_setup         err and status in one copy (flag_span)
//   mpcqp_update_batch  q, l, u back to back, then the error flags read back (update_bytes)
size_t input_span(const mpcqp_handle* h, const Shard& s) {
    return (size_t)((const char*)(s.in_u + s.B * h->m) - (const char*)s.in_Px);
}
size_t flag_span(const Shard& s) { return (size_t)((const char*)(s.kp.status + s.B) - (const char*)s.kp.err); }
size_t update_bytes(const mpcqp_handle* h, long Bs) {
    return sizeof(double) * (size_t)Bs * (h->n + 2 * h->m) + sizeof(int) * (size_t)Bs;
}
int need_hin(const mpcqp_handle* h, Shard& s) {
    if (s.hin) return 0;
    size_t by = std::max(update_bytes(h, s.B), flag_span(s));
    if (input_span(h, s) <= kStageMax) by = std::max(by, input_span(h, s));
    HIPCHK(pool_malloc(s.dev, by, (void**)&s.hin, true));
    s.hin_bytes = by;
    return 0;
}

// Everything a solve returns, one listing: the caller's array (ResultPtrs, null: not asked
// for), the device array, elements per instance, element size.  The segments lie back to back
// in this order in the shard's persistent pinned block hstage and its device twin dstage
// (launch_gather), filled by mpcqp_solve_batch with one synchronisation; the info / certificate
// / polish getters then read hstage (mpcqp_handle::staged).
struct ResultPtrs {
    void *x = nullptr, *y = nullptr, *obj = nullptr, *pri = nullptr, *dua = nullptr, *rho_est = nullptr,
         *dxc = nullptr, *dyc = nullptr, *status = nullptr, *iter = nullptr, *rho_upd = nullptr, *pstat = nullptr;
};
struct Results {
    Seg seg[kGatherMax];
    size_t nseg, bytes;
};
Results result_segs(const mpcqp_handle* h, const Shard& s, const ResultPtrs& u) {
    const long n = h->n, m = h->m;
    const KParams& k = s.kp;
    const Dir dn = Dir::down;
    Results r{{{u.x, s.out_x, n, 8, dn, 0}, {u.y, s.out_y, m, 8, dn, 0},
               {u.obj, k.obj, 1, 8, dn, 0}, {u.pri, k.pri, 1, 8, dn, 0}, {u.dua, k.dua, 1, 8, dn, 0},
               {u.rho_est, k.rho_est, 1, 8, dn, 0}, {u.dxc, k.dxc, n, 8, dn, 0}, {u.dyc, k.dyc, m, 8, dn, 0},
               {u.status, k.status, 1, 4, dn, 0}, {u.iter, k.iter, 1, 4, dn, 0}, {u.rho_upd, k.rho_upd, 1, 4, dn, 0},
               {u.pstat, h->set.polish ? k.pstat : nullptr, 1, 4, dn, 0}},  // (no polish: zeros)
              12, 0};
    for (size_t i = 0; i < r.nseg; ++i) {
        r.seg[i].off = r.bytes;
        r.bytes += seg_bytes(r.seg[i], s.B);
    }
    return r;
}
// the getters: out of hstage after a staged solve, else one synchronous copy per array
int read_results(mpcqp_handle* h, const ResultPtrs& u) {
    for (auto& s : h->shards) {
        if (!h->staged) HIPCHK(hipSetDevice(s.dev));
        const Results r = result_segs(h, s, u);
        if (h->staged) {
            stage_unpack(s, r.seg, r.nseg, s.hstage);
            continue;
        }
        for (size_t i = 0; i < r.nseg; ++i) {
            const Seg& g = r.seg[i];
            if (!g.host) continue;
            if (g.dev) HIPCHK(hipMemcpy(seg_host(g, s.b0), g.dev, seg_bytes(g, s.B), hipMemcpyDeviceToHost));
            else memset(seg_host(g, s.b0), 0, seg_bytes(g, s.B));
        }
    }
    return 0;
}

// osqp_setup's convexity test (OSQP 0.6 init_linsys_solver: the quasi-definite KKT matrix
// must have n positive pivots, which holds iff P + sigma I + A' diag(rho) A is positive
// definite -- the reduced matrix the solve kernels factor): one factor-only launch of the
// solve kernel per shard, which stops after the first factorisation and marks an instance
// whose factorisation fails as non-convex.  The first such instance is reported.
// The setup's invalid-data flags (check_err_flags) and osqp_setup's convexity test
// (check_convex) behind the setup kernel with one synchronisation: the factor-only launch is
// enqueued right after it, and both the flags and the statuses come back through the shard's
// pinned input block in stream order.  Invalid data is reported first, as the two checks in
// turn would.
int check_setup(mpcqp_handle* h) {
    const size_t ns = h->shards.size();
    std::vector<const int*> err(ns, nullptr), stat(ns, nullptr);
    std::vector<std::vector<int>> host(ns);
    for (size_t si = 0; si < ns; ++si) {
        Shard& s = h->shards[si];
        const int e = on_stream(s, s.stream, [&]() -> int {
            HIPCHK(launch_solve(s.kp, s.B, s.out_x, s.out_y, 1, s.stream));
            const size_t span = flag_span(s);
            if (std::max(span, update_bytes(h, s.B)) > kStageMax) return 0;
            if (int e = need_hin(h, s)) return e;
            HIPCHK(hipMemcpyAsync(s.hin, s.kp.err, span, hipMemcpyDeviceToHost, s.stream));
            err[si] = (const int*)s.hin;
            stat[si] = err[si] + (s.kp.status - s.kp.err);
            return 0;
        });
        if (e) return e;
    }
    if (int e = sync_all(h)) return e;
    for (size_t si = 0; si < ns; ++si) {
        Shard& s = h->shards[si];
        if (err[si]) continue;
        host[si].resize(2 * s.B);
        HIPCHK(hipSetDevice(s.dev));
        HIPCHK(hipMemcpy(host[si].data(), s.kp.err, sizeof(int) * s.B, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(host[si].data() + s.B, s.kp.status, sizeof(int) * s.B, hipMemcpyDeviceToHost));
        err[si] = host[si].data();
        stat[si] = err[si] + s.B;
    }
    for (size_t si = 0; si < ns; ++si)
        if (int e = first_flagged(err[si], h->shards[si].B, h->shards[si].b0)) return e;
    for (size_t si = 0; si < ns; ++si)
        if (int e = first_nonconvex(stat[si], h->shards[si].B, h->shards[si].b0)) return e;
    return 0;
}

int check_convex(mpcqp_handle* h) {
    for (auto& s : h->shards)
        if (int e = on_stream(s, s.stream, [&]() -> int {
                HIPCHK(launch_solve(s.kp, s.B, s.out_x, s.out_y, 1, s.stream));
                return 0;
            }))
            return e;
    if (int e = sync_all(h)) return e;
    for (auto& s : h->shards) {
        std::vector<int> st(s.B);
        HIPCHK(hipSetDevice(s.dev));
        HIPCHK(hipMemcpy(st.data(), s.kp.status, sizeof(int) * s.B, hipMemcpyDeviceToHost));
        if (int e = first_nonconvex(st.data(), s.B, s.b0)) return e;
    }
    return 0;
}

void free_shard(Shard& s) {
    (void)hipSetDevice(s.dev);
    if (s.stream) (void)hipStreamSynchronize(s.stream);
    if (s.last_st && s.last_st != s.stream && s.last_ev)
        (void)hipEventSynchronize(s.last_ev);  // a caller stream's last call
    pool_free(s.dev, s.dws_bytes, s.dws, false);
    pool_free(s.dev, s.dplan_bytes, s.dplan, false, s.dplan_tag);
    pool_free(s.dev, s.hstage_bytes, s.hstage, true);
    pool_free(s.dev, s.dstage_bytes, s.dstage, false);
    pool_free(s.dev, s.hin_bytes, s.hin, true);
    pool_stream_release(s);
    s = Shard{};
}

// Move a handle whose plan eliminated variables (choose_plan: the slack layouts) onto the
// plain plan, keeping its state, so that polish -- whose factorisation covers all of K
// (factorize<POL>) -- can run (osqp-python's update_settings(polish=True) at any time).
// Everything a solve carries from call to call moves over unchanged: the scaled data and
// the scaling, the iterates x, z, y, each instance's rho and row classes, its last status,
// info and certificates, the setup inputs; the per-column arrays (q, D, x: padded order)
// are permuted from the old padded index to the new one, and the scaled A values from the
// old plan's padded-CSC order to the new one's.  The factor is formed at the start
// of every solve, so nothing of it is kept.  The dispatch order restarts in identity order.
int replan_plain(mpcqp_handle* h) {
    if (int e = sync_all(h)) return e;
    mpcqp_settings st = h->set;
    st.polish = 1;
    auto npl = std::make_shared<Plan>();
    std::string err = choose_plan(h->n, h->m, h->Pp.data(), h->Pi.data(), h->Ap.data(), h->Ai.data(), st, *npl);
    if (!err.empty()) return fail(MPCQP_EUNSUPPORTED, "re-plan for polish: %s", err.c_str());
    std::shared_ptr<const Plan> oldp = h->plan;
    const Plan& old = *oldp;
    h->plan = npl;
    const long n = h->n;
    // one region across, by the listing's rule for it (workspace_regions)
    auto move = [&](const Region& a, const Region& b, long B) -> int {
        double *src = (double*)region_ptr(a), *dst = (double*)region_ptr(b);
        if (a.carry == Carry::drop || !a.count || !src || !dst) return 0;
        if (a.carry == Carry::copy) {
            HIPCHK(hipMemcpy(dst, src, a.esz * a.count, hipMemcpyDeviceToDevice));
            return 0;
        }
        const long wo = (long)a.count / B, wn = (long)b.count / B;  // an instance's row, old and new
        std::vector<double> ho(a.count), hn(b.count, b.pad);
        if (hipMemcpy(ho.data(), src, sizeof(double) * a.count, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(MPCQP_EDEVICE, "re-plan: copy-out failed");
        const bool var = a.carry == Carry::by_var;  // else the padded-CSC order of each plan
        const std::vector<int>&from = var ? old.var_pad : old.csc_pos, &to = var ? npl->var_pad : npl->csc_pos;
        const long cols = var ? n : wo;  // (k.Ax[e] = Ax[acsc_v[e]], kernels.hip::k_setup: user value v at csc_pos[v])
        for (long i = 0; i < B; ++i)
            for (long j = 0; j < cols; ++j) hn[i * wn + to[j]] = ho[i * wo + from[j]];
        if (hipMemcpy(dst, hn.data(), sizeof(double) * b.count, hipMemcpyHostToDevice) != hipSuccess)
            return fail(MPCQP_EDEVICE, "re-plan: copy-in failed");
        return 0;
    };
    std::vector<Shard> fresh;
    fresh.reserve(h->shards.size());
    int rc = 0;
    for (auto& os : h->shards) {
        Shard s;
        s.dev = os.dev; s.b0 = os.b0; s.B = os.B;
        fresh.push_back(s);
        Shard& ns = fresh.back();
        const bool with_io = os.in_Px != nullptr;
        if ((rc = alloc_shard(h, ns, with_io))) break;
        ns.kp.mat_shared = os.kp.mat_shared;
        carry_settings(ns.kp, os.kp);
        const std::vector<Region> ra = workspace_regions(old, os.B, with_io, os),
                                  rb = workspace_regions(*npl, ns.B, with_io, ns);
        for (size_t i = 0; i < ra.size() && !rc; ++i) rc = move(ra[i], rb[i], os.B);
        if (rc) break;
        (void)hipSetDevice(ns.dev);
        if (hipMemcpy((void*)ns.kp.self, &ns.kp, sizeof(KParams), hipMemcpyHostToDevice) != hipSuccess) {
            rc = fail(MPCQP_EDEVICE, "re-plan: parameter copy failed");
            break;
        }
    }
    if (rc) {  // the handle keeps its old plan and workspace
        for (auto& s : fresh) free_shard(s);
        h->plan = oldp;
        return rc;
    }
    for (auto& s : h->shards) free_shard(s);
    h->shards.swap(fresh);
    h->staged = false;
    return 0;
}

// ---- the *_device entry points ----
int single_device(const mpcqp_handle* h) {
    if (!h || h->shards.size() != 1) return fail(MPCQP_EINVAL, "device entry points need a single-device handle");
    return 0;
}
// body(shard, stream) on the caller's stream (null: the handle's own), after the checks every
// device call makes; the entry points with checks of their own go to on_stream themselves
template <class F>
int on_caller_stream(mpcqp_handle* h, void* stream, F&& body) {
    Shard& s = h->shards[0];
    const hipStream_t st = stream ? (hipStream_t)stream : s.stream;
    return on_stream(s, st, [&]() -> int { return body(s, st); });
}
// what: the entry point reads the workspace's state (need_state), null: it does not
template <class F>
int device_call(mpcqp_handle* h, void* stream, const char* what, F&& body) {
    if (what)
        if (int e = need_state(h, what)) return e;
    if (int e = single_device(h)) return e;
    h->staged = false;  // (device work: the staged results of the last solve are stale)
    return on_caller_stream(h, stream, body);
}

// A launch between a fresh hipEvent pair, recorded in v, while `on` (collect: solve launches,
// collect_setup: setup launches); last: the pair mpcqp_last_kernel_ms reads.  No event between
// the kernels unless timing is on: every recorded event is a packet the command processor
// completes between two launches (≈12 us per step measured on the cfg-2 bench, 2.33 -> 2.40 M
// solves/s without them).
template <class F>
int timed_launch(bool on, std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, hipStream_t st,
                 std::pair<hipEvent_t, hipEvent_t>* last, F&& launch) {
    if (on) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreate(&a));
        HIPCHK(hipEventCreate(&b));
        HIPCHK(hipEventRecord(a, st));
        v.push_back({a, b});
    }
    if (int e = launch()) return e;
    if (on) {
        HIPCHK(hipEventRecord(v.back().second, st));
        if (last) *last = v.back();
    }
    return 0;
}

}  // namespace

extern "C" {

void mpcqp_default_settings(mpcqp_settings* s) {
    s->rho = 0.1; s->sigma = 1e-6; s->alpha = 1.6;
    s->eps_abs = 1e-3; s->eps_rel = 1e-3; s->eps_prim_inf = 1e-4; s->eps_dual_inf = 1e-4;
    s->adaptive_rho_tolerance = 5.0;
    s->max_iter = 4000; s->scaling = 10; s->check_termination = 25; s->warm_start = 1;
    s->adaptive_rho = 1; s->adaptive_rho_interval = 0; s->scaled_termination = 0; s->polish = 0;
    s->verbose = 0; s->delta = 1e-6; s->polish_refine_iter = 3;
}

const char* mpcqp_last_error(void) { return g_err.c_str(); }

int mpcqp_analyze(int32_t n, int32_t m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                  const int32_t* Ai, int32_t* nb, int32_t* block, int32_t* var_pad, int32_t* bsize) {
    return mpcqp_analyze_ex(n, m, Pp, Pi, Ap, Ai, 0, nb, block, var_pad, bsize, nullptr);
}

int mpcqp_analyze_ex(int32_t n, int32_t m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                     const int32_t* Ai, int32_t eliminate, int32_t* nb, int32_t* block, int32_t* var_pad,
                     int32_t* bsize, int32_t* n_eliminated) {
    Plan pl;
    std::string err = build_plan(n, m, Pp, Pi, Ap, Ai, pl, eliminate != 0, !eliminate);
    if (n_eliminated) *n_eliminated = pl.ne;
    if (!err.empty()) return fail(err.rfind("unsupported", 0) == 0 ? MPCQP_EUNSUPPORTED : MPCQP_EINVAL, "%s", err.c_str());
    if (nb) *nb = pl.nb;
    if (block) *block = kS;
    if (var_pad) std::copy(pl.var_pad.begin(), pl.var_pad.end(), var_pad);
    if (bsize) std::copy(pl.bsize.begin(), pl.bsize.end(), bsize);
    return 0;
}

int mpcqp_setup_batch(int32_t n, int32_t m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                      const int32_t* Ai, int64_t B, const double* Px, const double* Ax, const double* q,
                      const double* l, const double* u, const mpcqp_settings* settings,
                      uint32_t device_mask, mpcqp_handle** out) {
    if (!Px || !Ax || !q || !l || !u) return fail(MPCQP_EINVAL, "NULL data array");
    std::vector<int> devs;
    for (int d = 0; d < 32; ++d)
        if (device_mask & (1u << d)) devs.push_back(d);
    if (devs.empty()) devs.push_back(0);
    // MPCQP_SPLIT=k (diagnostic): k contiguous shards per selected device, each with its own
    // stream, workspace and dispatch order -- the multi-device shard / gather code (b0
    // offsets, launch-all-then-gather) exercised on a one-GPU box
    if (const char* ev = getenv("MPCQP_SPLIT"); ev && atoi(ev) > 1) {
        const int k = std::min(atoi(ev), 64);
        std::vector<int> rep;
        for (int d : devs)
            for (int i = 0; i < k; ++i) rep.push_back(d);
        devs.swap(rep);
    }
    mpcqp_handle* h = nullptr;
    if (int e = make_handle(n, m, Pp, Pi, Ap, Ai, B, settings, devs, true, &h)) return e;
    if (int e = check_bounds_host(h, l, u, B)) { mpcqp_free(h); return e; }
    const Plan& pl = *h->plan;
    // the five inputs lie one after another in the workspace (workspace_regions): a small shard
    // stages them in pinned memory with the same layout and goes up in one copy (five pageable
    // copies cost ~4 us each on a one-QP setup)
    auto upload = [&](Shard& s) -> int {
        return on_stream(s, s.stream, [&]() -> int {
            auto at = [&](const double* d) { return (size_t)((const char*)d - (const char*)s.in_Px); };
            const Seg sg[] = {{(void*)Px, s.in_Px, pl.nnzP, 8, Dir::up, at(s.in_Px)},
                              {(void*)Ax, s.in_Ax, pl.nnzA, 8, Dir::up, at(s.in_Ax)},
                              {(void*)q, s.in_q, n, 8, Dir::up, at(s.in_q)},
                              {(void*)l, s.in_l, m, 8, Dir::up, at(s.in_l)},
                              {(void*)u, s.in_u, m, 8, Dir::up, at(s.in_u)}};
            const bool staged = input_span(h, s) <= kStageMax;
            if (staged)
                if (int e = need_hin(h, s)) return e;
            if (int e = stage_up(s, sg, 5, staged ? s.hin : nullptr, s.in_Px)) return e;
            HIPCHK(launch_setup(s.kp, s.B, s.in_Px, s.in_Ax, s.in_q, s.in_l, s.in_u, s.stream));
            return 0;
        });
    };
    strace().mark("handle");
    for (auto& s : h->shards)
        if (int e = upload(s)) { mpcqp_free(h); return e; }
    strace().mark("inputs + setup launch");
    if (int e = check_setup(h)) { mpcqp_free(h); return e; }
    strace().mark("setup + convexity wait");
    h->has_setup = true;
    *out = h;
    return 0;
}

int mpcqp_update_batch(mpcqp_handle* h, const double* q, const double* l, const double* u) {
    if (int e = need_state(h, "mpcqp_update_batch")) return e;
    if (!h) return fail(MPCQP_EINVAL, "NULL handle");
    h->staged = false;  // (device work: the staged results of the last solve are stale)
    if (l && u)
        if (int e = check_bounds_host(h, l, u, h->B)) return e;
    const long n = h->n, m = h->m;
    // small shards go through pinned staging (Shard::hin): the copies and the error flags'
    // read-back are asynchronous and the call synchronises once (osqp's per-step update of one
    // problem); the device arrays are not one run, so one copy per array either way.  In hin: q,
    // l, u back to back, then the flags (update_bytes)
    auto staged = [&](const Shard& s) { return update_bytes(h, s.B) <= kStageMax; };
    auto at = [&](const Shard& s, long doubles) { return sizeof(double) * (size_t)s.B * doubles; };
    auto flags = [&](const Shard& s) { return (int*)(s.hin + at(s, n + 2 * m)); };
    for (auto& s : h->shards) {
        const int rc = on_stream(s, s.stream, [&]() -> int {
            const Seg sg[] = {{(void*)q, s.in_q, n, 8, Dir::up, at(s, 0)},
                              {(void*)l, s.in_l, m, 8, Dir::up, at(s, n)},
                              {(void*)u, s.in_u, m, 8, Dir::up, at(s, n + m)}};
            if (staged(s))
                if (int e = need_hin(h, s)) return e;
            if (int e = stage_up(s, sg, 3, staged(s) ? s.hin : nullptr, nullptr)) return e;
            HIPCHK(launch_update(s.kp, s.B, q ? s.in_q : nullptr, l ? s.in_l : nullptr, u ? s.in_u : nullptr, s.stream));
            if (staged(s) && (l || u))
                HIPCHK(hipMemcpyAsync(flags(s), s.kp.err, sizeof(int) * s.B, hipMemcpyDeviceToHost, s.stream));
            return 0;
        });
        if (rc) return rc;
    }
    if (int e = sync_all(h)) return e;
    if (!(l || u)) return 0;
    for (auto& s : h->shards)
        if (int e = staged(s) ? first_flagged(flags(s), s.B, s.b0) : shard_err_flags(s)) return e;
    return 0;
}

int mpcqp_update_matrices_batch(mpcqp_handle* h, const double* Px, const int32_t* Px_idx, int32_t nPx,
                                const double* Ax, const int32_t* Ax_idx, int32_t nAx) {
    if (int e = need_state(h, "mpcqp_update_matrices_batch")) return e;
    if (!h) return fail(MPCQP_EINVAL, "NULL handle");
    h->staged = false;  // (device work: the staged results of the last solve are stale)
    if (!Px && !Ax) return fail(MPCQP_EINVAL, "no matrix values given");
    const Plan& pl = *h->plan;
    // the columns of the value arrays that are written: all, or per index its last
    // occurrence (OSQP's sequential loop: a repeated index takes the last value)
    auto pick_cols = [&](const int32_t* idx, int32_t k, int nnz, const char* name, std::vector<int>& col,
                         std::vector<int>& dst) -> int {
        if (!idx) {
            col.resize(nnz);
            for (int i = 0; i < nnz; ++i) col[i] = i;
            dst = col;
            return 0;
        }
        if (k < 0 || k > nnz)
            return fail(MPCQP_EINVAL, "new number of elements (%d) greater than elements in %s (%d)", k, name, nnz);
        std::vector<int> last(nnz, -1);
        for (int i = 0; i < k; ++i) {
            if (idx[i] < 0 || idx[i] >= nnz) return fail(MPCQP_EINVAL, "%s index %d out of range", name, idx[i]);
            last[idx[i]] = i;
        }
        for (int v = 0; v < nnz; ++v)
            if (last[v] >= 0) { col.push_back(last[v]); dst.push_back(v); }
        return 0;
    };
    std::vector<int> pcol, pdst, acol, adst;
    if (Px)
        if (int e = pick_cols(Px_idx, nPx, pl.nnzP, "P", pcol, pdst)) return e;
    if (Ax)
        if (int e = pick_cols(Ax_idx, nAx, pl.nnzA, "A", acol, adst)) return e;
    const int kP = Px ? (Px_idx ? nPx : pl.nnzP) : 0, kA = Ax ? (Ax_idx ? nAx : pl.nnzA) : 0;
    const int nP = (int)pdst.size(), nA = (int)adst.size();
    for (auto& s : h->shards) {
        if (!s.in_Px) return fail(MPCQP_EINVAL, "matrix updates need a handle made by mpcqp_setup_batch");
        if (s.kp.mat_shared) return fail(MPCQP_EINVAL, "matrix updates need per-instance matrices (shared mode is on)");
    }
    // per shard: the selected values (Bs x nP, Bs x nA) and their indices, in one staging
    // allocation freed after the call
    std::vector<void*> tmp(h->shards.size(), nullptr);
    auto release = [&]() {
        for (size_t i = 0; i < tmp.size(); ++i)
            if (tmp[i]) { (void)hipSetDevice(h->shards[i].dev); (void)hipFree(tmp[i]); }
    };
    int err = 0;
    std::vector<std::vector<double>> host(h->shards.size());
    for (size_t si = 0; si < h->shards.size() && !err; ++si) {
        Shard& s = h->shards[si];
        const long Bs = s.B;
        std::vector<double>& hv = host[si];
        hv.resize((size_t)Bs * (nP + nA));
        for (long b = 0; b < Bs; ++b) {
            for (int k = 0; k < nP; ++k) hv[b * nP + k] = Px[(s.b0 + b) * kP + pcol[k]];
            for (int k = 0; k < nA; ++k) hv[Bs * nP + b * nA + k] = Ax[(s.b0 + b) * kA + acol[k]];
        }
        const size_t vbytes = sizeof(double) * hv.size(), ibytes = sizeof(int) * (size_t)(nP + nA);
        err = on_stream(s, s.stream, [&]() -> int {
            HIPCHK(hipMalloc(&tmp[si], vbytes + ibytes + 16));
            double* dv = (double*)tmp[si];
            int* di = (int*)((char*)tmp[si] + vbytes);
            if (vbytes) HIPCHK(hipMemcpyAsync(dv, hv.data(), vbytes, hipMemcpyHostToDevice, s.stream));
            if (nP) HIPCHK(hipMemcpyAsync(di, pdst.data(), sizeof(int) * nP, hipMemcpyHostToDevice, s.stream));
            if (nA) HIPCHK(hipMemcpyAsync(di + nP, adst.data(), sizeof(int) * nA, hipMemcpyHostToDevice, s.stream));
            HIPCHK(launch_update_mat(s.kp, Bs, s.in_Px, s.in_Ax, s.in_q, s.in_l, s.in_u, Px ? dv : nullptr, di, nP,
                                     Ax ? dv + Bs * nP : nullptr, di + nP, nA, s.stream));
            return 0;
        });
    }
    if (!err) err = sync_all(h);
    release();
    if (err) return err;
    if (int e = check_err_flags(h)) return e;
    return check_convex(h);  // osqp_update_P_A refactors at once and reports a failed factorisation
}

int mpcqp_update_settings(mpcqp_handle* h, const mpcqp_settings* s, int32_t set_rho) {
    if (!h || !s) return fail(MPCQP_EINVAL, "NULL argument");
    h->staged = false;  // (device work: the staged results of the last solve are stale)
    const mpcqp_settings& o = h->set;
    if (s->sigma != o.sigma || s->scaling != o.scaling || s->adaptive_rho != o.adaptive_rho ||
        s->adaptive_rho_tolerance != o.adaptive_rho_tolerance || s->adaptive_rho_interval != o.adaptive_rho_interval)
        return fail(MPCQP_EINVAL, "sigma, scaling and the adaptive-rho settings cannot be changed after setup");
    if (int e = validate_settings(*s)) return e;  // (polish's delta / refinement steps included)
    if (s->polish && h->plan->ne > 0)  // polish factors all of K: the plain plan, state kept
        if (int e = replan_plain(h)) return e;
    const bool rho_changed = set_rho != 0;
    const double rho = std::min(std::max(s->rho, 1e-6), 1e6);  // osqp_update_rho: RHO_MIN / RHO_MAX
    for (auto& sh : h->shards) {
        KParams& k = sh.kp;
        apply_settings(k, *s);
        const int rc = on_stream(sh, sh.stream, [&]() -> int {
            HIPCHK(hipMemcpyAsync((void*)k.self, &k, sizeof(KParams), hipMemcpyHostToDevice, sh.stream));
            if (rho_changed) {  // every instance's current rho (scal[2]); the solve refactors with it
                HIPCHK(hipMemsetAsync(k.ffresh, 0, sizeof(int) * sh.B, sh.stream));
                std::vector<double> r(sh.B, rho);
                HIPCHK(hipMemcpy2DAsync(k.scal + 2, 4 * sizeof(double), r.data(), sizeof(double), sizeof(double), sh.B,
                                        hipMemcpyHostToDevice, sh.stream));
                HIPCHK(hipStreamSynchronize(sh.stream));  // r is a host temporary
            }
            return 0;
        });
        if (rc) return rc;
    }
    const int interval = h->set.adaptive_rho_interval;
    h->set = *s;
    h->set.adaptive_rho_interval = interval;
    return sync_all(h);
}

int mpcqp_warm_start_batch(mpcqp_handle* h, const double* x, const double* y) {
    if (int e = need_state(h, "mpcqp_warm_start_batch")) return e;
    if (!h) return fail(MPCQP_EINVAL, "NULL handle");
    h->staged = false;  // (device work: the staged results of the last solve are stale)
    const long n = h->n, m = h->m;
    for (auto& s : h->shards) {
        const int rc = on_stream(s, s.stream, [&]() -> int {
            if (x) HIPCHK(hipMemcpyAsync(s.out_x, x + s.b0 * n, sizeof(double) * s.B * n, hipMemcpyHostToDevice, s.stream));
            if (y) HIPCHK(hipMemcpyAsync(s.out_y, y + s.b0 * m, sizeof(double) * s.B * m, hipMemcpyHostToDevice, s.stream));
            HIPCHK(launch_warm(s.kp, s.B, x ? s.out_x : nullptr, y ? s.out_y : nullptr, s.stream));
            return 0;
        });
        if (rc) return rc;
        s.kp.warm_start = 1;
    }
    h->set.warm_start = 1;
    return sync_all(h);
}

int mpcqp_solve_batch(mpcqp_handle* h, double* x, double* y, int32_t* status, int32_t* iters) {
    if (int e = need_state(h, "mpcqp_solve_batch")) return e;
    if (!h) return fail(MPCQP_EINVAL, "NULL handle");
    // every shard's kernels are enqueued before any result is copied back: a copy into the
    // caller's (pageable) memory blocks the host until its shard is done, so copying inside
    // the launch loop would start shard d+1 only after shard d had finished
    // an event pair around the solve launch only while timing is on (mpcqp_timing): two event
    // packets cost a one-QP solve() ~5.5 us of its ~150 (cfg 2, same-box A/B, profiles/r6/lat_events_ab.txt)
    const bool evs = h->collect;
    for (auto& s : h->shards) {
        const int rc = on_stream(s, s.stream, [&]() -> int {
            if (evs) HIPCHK(hipEventRecord(s.ev0, s.stream));
            HIPCHK(launch_solve(s.kp, s.B, s.out_x, s.out_y, 0, s.stream));
            if (evs) HIPCHK(hipEventRecord(s.ev1, s.stream));
            HIPCHK(launch_order(s.kp, s.B, s.stream));
            return 0;
        });
        if (rc) return rc;
    }
    // the host-side gather: each shard's slice of the caller's buffers, in shard order; a
    // small shard stages everything its solve returns in pinned memory (one synchronisation
    // for the solve and the getters that follow it, instead of one per array): one gather
    // kernel into the device twin of the staging layout, one copy down
    ResultPtrs u;
    u.x = x; u.y = y; u.status = status; u.iter = iters;
    bool all_staged = true;
    for (auto& s : h->shards) {
        HIPCHK(hipSetDevice(s.dev));
        const Results r = result_segs(h, s, u);
        const bool staged = r.bytes <= kStageMax;
        if (staged) {
            if (!s.hstage) {
                HIPCHK(pool_malloc(s.dev, r.bytes, (void**)&s.hstage, true));
                s.hstage_bytes = r.bytes;
            }
            if (!s.dstage) {
                HIPCHK(pool_malloc(s.dev, r.bytes, (void**)&s.dstage, false));
                s.dstage_bytes = r.bytes;
            }
            GatherList gl{};
            for (size_t i = 0; i < r.nseg; ++i) {
                const Seg& g = r.seg[i];
                gl.seg[gl.nseg++] = GatherSeg{g.dev, (long)g.off, s.B * g.per, g.sz};
                gl.most = std::max(gl.most, s.B * g.per);
            }
            HIPCHK(launch_gather(gl, s.dstage, s.stream));
        } else {
            all_staged = false;
        }
        if (int e = stage_down(s, r.seg, r.nseg, staged ? s.hstage : nullptr, s.dstage, r.bytes)) return e;
    }
    if (int e = sync_all(h)) return e;
    for (auto& s : h->shards) {
        const Results r = result_segs(h, s, u);
        if (r.bytes <= kStageMax) stage_unpack(s, r.seg, r.nseg, s.hstage);
    }
    h->staged = all_staged;
    h->solved = true;
    float ms = 0.f;
    h->last_ms = -1.0;
    if (evs && h->shards.size() == 1 && hipEventElapsedTime(&ms, h->shards[0].ev0, h->shards[0].ev1) == hipSuccess) {
        h->last_ms = ms;
        h->last_pair = {h->shards[0].ev0, h->shards[0].ev1};
    }
    return 0;
}

int mpcqp_get_info_batch(mpcqp_handle* h, double* obj_val, double* pri_res, double* dua_res,
                         double* rho_estimate, int32_t* rho_updates) {
    if (!h) return fail(MPCQP_EINVAL, "NULL handle");
    ResultPtrs u;
    u.obj = obj_val; u.pri = pri_res; u.dua = dua_res; u.rho_est = rho_estimate; u.rho_upd = rho_updates;
    return read_results(h, u);
}

int mpcqp_get_polish_status(mpcqp_handle* h, int32_t* status_polish) {
    if (!h || !status_polish) return fail(MPCQP_EINVAL, "NULL argument");
    ResultPtrs u;
    u.pstat = status_polish;
    return read_results(h, u);
}

int mpcqp_get_certificates(mpcqp_handle* h, double* prim_inf_cert, double* dual_inf_cert) {
    if (int e = need_state(h, "mpcqp_get_certificates")) return e;
    if (!h) return fail(MPCQP_EINVAL, "NULL handle");
    ResultPtrs u;
    u.dyc = prim_inf_cert; u.dxc = dual_inf_cert;
    return read_results(h, u);
}

int mpcqp_create(int32_t n, int32_t m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                 const int32_t* Ai, int64_t B, const mpcqp_settings* settings, int32_t device,
                 mpcqp_handle** out) {
    return make_handle(n, m, Pp, Pi, Ap, Ai, B, settings, std::vector<int>{device}, false, out);
}

// A setup overwrites the workspace: state_gone holds from before the launch (one that fails
// part-way leaves nothing a later call may read) until the setup is known to keep its state.
int mpcqp_setup_device(mpcqp_handle* h, const double* dPx, const double* dAx, const double* dq,
                       const double* dl, const double* du, void* stream) {
    return device_call(h, stream, nullptr, [&](Shard& s, hipStream_t st) -> int {
        h->state_gone = true;
        if (int e = timed_launch(h->collect_setup, h->ev_setup, st, nullptr,
                                 [&]() -> int { HIPCHK(launch_setup(s.kp, s.B, dPx, dAx, dq, dl, du, st)); return 0; }))
            return e;
        h->state_gone = false;
        h->solved = false;
        h->has_setup = true;
        return 0;
    });
}

int mpcqp_update_device(mpcqp_handle* h, const double* dq, const double* dl, const double* du, void* stream) {
    return device_call(h, stream, "mpcqp_update_device", [&](Shard& s, hipStream_t st) -> int {
        HIPCHK(launch_update(s.kp, s.B, dq, dl, du, st));
        return 0;
    });
}

int mpcqp_warm_start_device(mpcqp_handle* h, const double* dx, const double* dy, void* stream) {
    return device_call(h, stream, "mpcqp_warm_start_device", [&](Shard& s, hipStream_t st) -> int {
        HIPCHK(launch_warm(s.kp, s.B, dx, dy, st));
        s.kp.warm_start = 1;
        h->set.warm_start = 1;
        return 0;
    });
}

int mpcqp_setup_warm_device(mpcqp_handle* h, const double* dPx, const double* dAx, const double* dq,
                            const double* dl, const double* du, const double* dx0, const double* dy0, void* stream) {
    return device_call(h, stream, nullptr, [&](Shard& s, hipStream_t st) -> int {
        h->state_gone = true;
        if (int e = timed_launch(h->collect_setup, h->ev_setup, st, nullptr, [&]() -> int {
                HIPCHK(launch_setup_warm(s.kp, s.B, dPx, dAx, dq, dl, du, dx0, dy0, st));
                return 0;
            }))
            return e;
        h->state_gone = false;
        h->solved = false;
        h->has_setup = true;
        s.kp.warm_start = 1;
        h->set.warm_start = 1;
        return 0;
    });
}

int mpcqp_setup_warm_fused(const mpcqp_handle* h) {
    if (!h || h->shards.empty()) return fail(MPCQP_EINVAL, "mpcqp_setup_warm_fused: null handle");
    return setup_warm_fused(h->shards[0].kp) ? 1 : 0;
}

int mpcqp_solve_device(mpcqp_handle* h, double* dx, double* dy, int32_t* dstatus, int32_t* diters, void* stream) {
    return device_call(h, stream, "mpcqp_solve_device", [&](Shard& s, hipStream_t st) -> int {
        KParams k = s.kp;  // the solve kernel writes status / iter into the caller's arrays as well
        k.ostat = dstatus;
        k.oiter = diters;
        if (int e = timed_launch(h->collect, h->ev_solve, st, &h->last_pair,
                                 [&]() -> int { HIPCHK(launch_solve(k, s.B, dx, dy, 0, st)); return 0; }))
            return e;
        HIPCHK(launch_order(k, s.B, st));
        h->timed = true;
        h->solved = true;
        return 0;
    });
}

int mpcqp_setup_solve_device(mpcqp_handle* h, const double* dPx, const double* dAx, const double* dq,
                             const double* dl, const double* du, double* dx, double* dy, int32_t* dstatus,
                             int32_t* diters, void* stream) {
    return device_call(h, stream, nullptr, [&](Shard& s, hipStream_t st) -> int {
        KParams k = s.kp;
        k.ostat = dstatus;
        k.oiter = diters;
        const bool one = h->one_shot && one_shot_form(k) > 0;
        h->state_gone = one;
        if (int e = timed_launch(h->collect, h->ev_solve, st, &h->last_pair, [&]() -> int {
                HIPCHK(launch_setup_solve(k, s.B, dPx, dAx, dq, dl, du, dx, dy, st,
                                          one ? h->one_shot_loop : OneShot::off));
                return 0;
            }))
            return e;
        h->has_setup = true;
        HIPCHK(launch_order(k, s.B, st));
        h->timed = true;
        h->solved = true;
        return 0;
    });
}

// what the adjoint and solution-record entry points check before any device work: a finished
// solve (need_solved) or at least a setup; a handle on an eliminated plan then moves to the plain
// plan (the adjoint system is factored over all of K, as polish's)
static int need_plain_state(mpcqp_handle* h, bool need_solved, const char* what) {
    if (int e = need_state(h, what)) return e;
    if (need_solved && !h->solved)
        return fail(MPCQP_EINVAL, "%s: no solve has run on this handle's setup yet", what);
    if (!need_solved && !h->has_setup) return fail(MPCQP_EINVAL, "%s: no setup has run on this handle yet", what);
    if (h->plan->ne > 0)
        if (int e = replan_plain(h)) return e;
    return 0;
}
static int adjoint_enter(mpcqp_handle* h, int32_t nrhs, const void* gx, const void* gy, const char* what) {
    if (!h) return fail(MPCQP_EINVAL, "%s: NULL handle", what);
    if (nrhs < 1) return fail(MPCQP_EINVAL, "%s: nrhs must be at least 1 (got %d)", what, (int)nrhs);
    if (!gx && !gy) return fail(MPCQP_EINVAL, "%s: both seeds are NULL", what);
    return need_plain_state(h, true, what);
}

int mpcqp_adjoint_device(mpcqp_handle* h, int32_t nrhs, const double* dgx, const double* dgy, double* drx,
                         double* dry, double* dgq, double* dgl, double* dgu, double* dgPx, double* dgAx,
                         int8_t* dact, double* dares, int32_t* dastat, void* stream) {
    if (int e = adjoint_enter(h, nrhs, dgx, dgy, "mpcqp_adjoint_device")) return e;
    if (int e = single_device(h)) return e;
    return on_caller_stream(h, stream, [&](Shard& s, hipStream_t st) -> int {
        const AdjointIO io{nrhs, dgx, dgy, drx, dry, dgq, dgl, dgu, dgPx, dgAx, (signed char*)dact, dares, dastat};
        HIPCHK(launch_adjoint(s.kp, s.B, io, st));
        return 0;
    });
}

int mpcqp_adjoint_batch(mpcqp_handle* h, int32_t nrhs, const double* gx, const double* gy, double* rx, double* ry,
                        double* gq, double* gl, double* gu, double* gPx, double* gAx, int8_t* act, double* ares,
                        int32_t* astat) {
    if (int e = adjoint_enter(h, nrhs, gx, gy, "mpcqp_adjoint_batch")) return e;
    const long n = h->n, m = h->m, nP = h->plan->nnzP, nA = h->plan->nnzA, R = nrhs;
    // per shard one device block and (small shards) one pinned block of the same layout: the
    // seeds, then every output the caller asked for; freed (to the pool) after the call
    struct Tmp { void* d = nullptr; char* hb = nullptr; size_t bytes = 0; std::vector<Seg> sg; };
    std::vector<Tmp> tmp(h->shards.size());
    auto enqueue = [&](Shard& s, Tmp& t) -> int {
        t.sg = {{(void*)gx, nullptr, R * n, 8, Dir::up, 0}, {(void*)gy, nullptr, R * m, 8, Dir::up, 0},
                {rx, nullptr, R * n, 8, Dir::down, 0},      {ry, nullptr, R * m, 8, Dir::down, 0},
                {gq, nullptr, R * n, 8, Dir::down, 0},      {gl, nullptr, R * m, 8, Dir::down, 0},
                {gu, nullptr, R * m, 8, Dir::down, 0},      {gPx, nullptr, R * nP, 8, Dir::down, 0},
                {gAx, nullptr, R * nA, 8, Dir::down, 0},    {ares, nullptr, R, 8, Dir::down, 0},
                {astat, nullptr, 1, 4, Dir::down, 0},       {act, nullptr, m, 1, Dir::down, 0}};
        size_t end = 0;
        for (Seg& g : t.sg)
            if (g.host) g.off = carve(end, seg_bytes(g, s.B));
        t.bytes = end + 256;
        return on_stream(s, s.stream, [&]() -> int {
            HIPCHK(pool_malloc(s.dev, t.bytes, &t.d, false));
            if (t.bytes <= kStageMax) HIPCHK(pool_malloc(s.dev, t.bytes, (void**)&t.hb, true));
            for (Seg& g : t.sg)
                if (g.host) g.dev = (char*)t.d + g.off;
            if (int e = stage_up(s, t.sg.data(), t.sg.size(), t.hb, t.d)) return e;  // the seeds lie first
            auto dp = [&](int k) { return t.sg[k].dev; };
            const AdjointIO io{nrhs, (const double*)dp(0), (const double*)dp(1), (double*)dp(2), (double*)dp(3),
                               (double*)dp(4), (double*)dp(5), (double*)dp(6), (double*)dp(7), (double*)dp(8),
                               (signed char*)dp(11), (double*)dp(9), (int*)dp(10)};
            HIPCHK(launch_adjoint(s.kp, s.B, io, s.stream));
            return stage_down(s, t.sg.data(), t.sg.size(), t.hb, t.d, end);
        });
    };
    int err = 0;
    for (size_t si = 0; si < h->shards.size() && !err; ++si) err = enqueue(h->shards[si], tmp[si]);
    if (int e = sync_all(h); e && !err) err = e;  // (also on an error: no block goes back to the pool in use)
    for (size_t si = 0; si < h->shards.size(); ++si) {
        const Shard& s = h->shards[si];
        Tmp& t = tmp[si];
        if (!err && t.hb) stage_unpack(s, t.sg.data(), t.sg.size(), t.hb);
        pool_free(s.dev, t.bytes, t.d, false);
        pool_free(s.dev, t.bytes, t.hb, true);
    }
    return err;
}

// The solution record (mpcqp.h): what k_adjoint reads of a finished solve -- x~ by variable, z~, y~,
// the status -- out of the workspace and back into it.  Both move a handle on an eliminated plan to
// the plain plan first, as the adjoint does, so a record is the same whichever plan the solve ran on.
static int record_enter(mpcqp_handle* h, const double* drecord, bool need_solved, const char* what) {
    if (!h) return fail(MPCQP_EINVAL, "%s: NULL handle", what);
    if (!drecord) return fail(MPCQP_EINVAL, "%s: NULL record", what);
    if (int e = single_device(h)) return e;
    return need_plain_state(h, need_solved, what);
}

int mpcqp_save_solution_device(mpcqp_handle* h, double* drecord, void* stream) {
    if (int e = record_enter(h, drecord, true, "mpcqp_save_solution_device")) return e;
    return on_caller_stream(h, stream, [&](Shard& s, hipStream_t st) -> int {
        HIPCHK(launch_save_solution(s.kp, s.B, drecord, st));
        return 0;
    });
}

int mpcqp_load_solution_device(mpcqp_handle* h, const double* drecord, void* stream) {
    if (int e = record_enter(h, drecord, false, "mpcqp_load_solution_device")) return e;
    h->staged = false;  // (device work: the staged results of the last solve are stale)
    return on_caller_stream(h, stream, [&](Shard& s, hipStream_t st) -> int {
        HIPCHK(launch_load_solution(s.kp, s.B, drecord, st));
        h->solved = true;
        return 0;
    });
}

void* mpcqp_get_stream(const mpcqp_handle* h) {
    return (h && !h->shards.empty()) ? (void*)h->shards[0].stream : nullptr;
}

int mpcqp_set_one_shot(mpcqp_handle* h, int32_t on) {
    if (int e = single_device(h)) return e;
    h->one_shot = on != 0;
    return 0;
}

int mpcqp_one_shot_applies(const mpcqp_handle* h) {
    return (h && h->shards.size() == 1) ? one_shot_form(h->shards[0].kp) : 0;
}

int mpcqp_one_shot_kernel(const mpcqp_handle* h) {
    return (h && h->shards.size() == 1 && h->one_shot) ? one_shot_kernel(h->shards[0].kp, h->one_shot_loop) : -1;
}

int mpcqp_set_shared_matrices(mpcqp_handle* h, int32_t shared) {
    if (int e = single_device(h)) return e;
    h->staged = false;  // (device work: the staged results of the last solve are stale)
    h->shards[0].kp.mat_shared = shared ? 1 : 0;
    return 0;
}

int mpcqp_synchronize(mpcqp_handle* h) {
    if (!h) return fail(MPCQP_EINVAL, "NULL handle");
    return sync_all(h);
}

double mpcqp_last_kernel_ms(mpcqp_handle* h) {
    if (!h || h->shards.size() != 1 || !h->last_pair.first) return -1.0;
    Shard& s = h->shards[0];
    float ms = 0.f;
    if (hipSetDevice(s.dev) != hipSuccess) return -1.0;
    if (hipEventSynchronize(h->last_pair.second) != hipSuccess) return -1.0;
    if (hipEventElapsedTime(&ms, h->last_pair.first, h->last_pair.second) != hipSuccess) return -1.0;
    return ms;
}

static int drain(std::vector<std::pair<hipEvent_t, hipEvent_t>>& v, double* total) {
    double t = 0.0;
    for (auto& e : v) {
        float ms = 0.f;
        HIPCHK(hipEventSynchronize(e.second));
        HIPCHK(hipEventElapsedTime(&ms, e.first, e.second));
        t += ms;
        (void)hipEventDestroy(e.first);
        (void)hipEventDestroy(e.second);
    }
    if (total) *total = t;
    v.clear();
    return 0;
}

int mpcqp_timing(mpcqp_handle* h, int32_t enable) {
    if (!h || h->shards.size() != 1) return fail(MPCQP_EINVAL, "timing needs a single-device handle");
    if (int e = hipSetDevice(h->shards[0].dev) == hipSuccess ? 0 : fail(MPCQP_EDEVICE, "hipSetDevice")) return e;
    double t;
    if (int e = drain(h->ev_setup, &t)) return e;
    if (int e = drain(h->ev_solve, &t)) return e;
    h->last_pair = {nullptr, nullptr};  // the drained events are gone
    h->collect = (enable & 1) != 0;
    h->collect_setup = (enable & 2) != 0;
    return 0;
}

int mpcqp_timing_read(mpcqp_handle* h, double* setup_ms, int32_t* n_setup, double* solve_ms, int32_t* n_solve) {
    if (!h || h->shards.size() != 1) return fail(MPCQP_EINVAL, "timing needs a single-device handle");
    HIPCHK(hipSetDevice(h->shards[0].dev));
    if (n_setup) *n_setup = (int32_t)h->ev_setup.size();
    if (n_solve) *n_solve = (int32_t)h->ev_solve.size();
    if (int e = drain(h->ev_setup, setup_ms)) return e;
    if (int e = drain(h->ev_solve, solve_ms)) return e;
    h->last_pair = {nullptr, nullptr};
    return 0;
}

int mpcqp_get_plan_info(const mpcqp_handle* h, mpcqp_plan_info* info) {
    if (!h || !info) return fail(MPCQP_EINVAL, "NULL argument");
    fill_plan_info(info, h->n, h->m, *h->plan, h->shards.empty() ? nullptr : &h->shards[0].kp);
    info->batch = h->B; info->n_devices = (int)h->shards.size();
    return 0;
}

int mpcqp_plan_preview(int32_t n, int32_t m, const int32_t* Pp, const int32_t* Pi, const int32_t* Ap,
                       const int32_t* Ai, const mpcqp_settings* settings, mpcqp_plan_info* info, char* note,
                       int32_t note_cap) {
    if (!info || !Pp || !Pi || !Ap || !Ai) return fail(MPCQP_EINVAL, "NULL argument");
    mpcqp_settings st;
    if (settings) st = *settings;
    else mpcqp_default_settings(&st);
    if (int e = validate_settings(st)) return e;
    Plan pl;
    std::string err = choose_plan(n, m, Pp, Pi, Ap, Ai, st, pl);
    if (note && note_cap > 0) snprintf(note, (size_t)note_cap, "%s", pl.choice_note.c_str());
    if (!err.empty()) return fail(err.rfind("unsupported", 0) == 0 ? MPCQP_EUNSUPPORTED : MPCQP_EINVAL, "%s", err.c_str());
    KParams k{};
    shape_params(pl, k);
    if (int e = pick_variant(k)) return e;
    *info = mpcqp_plan_info{};
    fill_plan_info(info, n, m, pl, &k);
    return 0;
}

int mpcqp_debug_phase_times(mpcqp_handle* h, int64_t* out) {
    if (!h || !out) return fail(MPCQP_EINVAL, "NULL argument");
    for (auto& s : h->shards)
        if (!s.kp.prof) return fail(MPCQP_EINVAL, "phase timers not enabled (set MPCQP_PHASE_PROF=1 before create)");
    if (int e = sync_all(h)) return e;
    for (auto& s : h->shards) {
        HIPCHK(hipSetDevice(s.dev));
        HIPCHK(hipMemcpy(out + s.b0 * kProfSlots, s.kp.prof, sizeof(int64_t) * s.B * kProfSlots, hipMemcpyDeviceToHost));
    }
    return 0;
}

int mpcqp_debug_dispatch_order(mpcqp_handle* h, int32_t* out) {
    if (!h || !out) return fail(MPCQP_EINVAL, "NULL argument");
    if (int e = sync_all(h)) return e;
    for (auto& s : h->shards) {
        int32_t* o = out + s.b0;
        if (!s.kp.order) {
            for (long i = 0; i < s.B; ++i) o[i] = (int32_t)(s.b0 + i);
            continue;
        }
        HIPCHK(hipSetDevice(s.dev));
        HIPCHK(hipMemcpy(o, s.kp.order, sizeof(int32_t) * s.B, hipMemcpyDeviceToHost));
        for (long i = 0; i < s.B; ++i) o[i] += (int32_t)s.b0;
    }
    return 0;
}

int mpcqp_debug_copy(const double* src, double* dst, int64_t n, int32_t reps, void* stream, double* ms) {
    if (!src || !dst || !ms || n <= 0 || n % 16384 || reps <= 0 || ((uintptr_t)src | (uintptr_t)dst) & 15)
        return fail(MPCQP_EINVAL, "mpcqp_debug_copy: n > 0, n %% 16384 == 0, reps > 0, 16-byte aligned buffers");
    hipStream_t st = (hipStream_t)stream;
    if (st) {  // the events and kernels on the device the caller's stream belongs to
        int dev = 0;
        HIPCHK(hipStreamGetDevice(st, &dev));
        HIPCHK(hipSetDevice(dev));
    }
    struct Events {  // destroyed on every return path (HIPCHK returns early)
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() {
            if (a) (void)hipEventDestroy(a);
            if (b) (void)hipEventDestroy(b);
        }
    } ev;
    HIPCHK(hipEventCreate(&ev.a));
    HIPCHK(hipEventCreate(&ev.b));
    hipEvent_t a = ev.a, b = ev.b;
    double best = 0.0;
    for (int form = 0; form < 5; ++form) {  // the fastest of the five forms (kernels.hip::launch_copy16)
        HIPCHK(launch_copy16(src, dst, n, st, form));  // (warm-up)
        HIPCHK(hipEventRecord(a, st));
        for (int r = 0; r < reps; ++r) HIPCHK(launch_copy16(src, dst, n, st, form));
        HIPCHK(hipEventRecord(b, st));
        HIPCHK(hipEventSynchronize(b));
        float t = 0.0f;
        HIPCHK(hipEventElapsedTime(&t, a, b));
        const double per = (double)t / reps;
        if (form == 0 || per < best) best = per;
    }
    *ms = best;
    return 0;
}

void mpcqp_free(mpcqp_handle* h) {
    if (!h) return;
    if (!h->shards.empty() && hipSetDevice(h->shards[0].dev) == hipSuccess) {
        double t;
        drain(h->ev_setup, &t);
        drain(h->ev_solve, &t);
    }
    for (auto& s : h->shards) free_shard(s);
    delete h;
}

}  // extern "C"
