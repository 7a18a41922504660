// qg_run.hip — the one-shot calls of include/qgemul.h (qgemul_run*, qgemul_run_batched*, qgemul_run_sharded): host tensors in, host
// tensor out, one synchronous call.  Every single-device entry point fills a RunRequest and goes through run_one_shot.
#include <atomic>

#include "qg_api_int.h"

// ---- the one-shot call keeps a per-thread cache: context, the plan of the last request, grow-only device buffers ----
// The reference is a synchronous library that user code calls in loops; creating a stream, a plan table and eight device
// allocations per call cost 2.9 ms for the README's 4x4x4 example (tools/measure_run_latency.py).  The cache belongs to
// the calling thread and is never touched by another one; qgemul_run_release() frees it, and so does the end of the thread
// (RunCacheReaper below) — except once the process is exiting: a worker thread that is still alive or detached then may run its
// thread-local destructors after HIP has been torn down, so the reaper only forgets its pointers (g_shutting_down).
namespace {
struct RunCache {
    qgemul_ctx* ctx = nullptr;
    int device = -2;
    qgemul_plan* plan = nullptr;
    QRunKey key;              // what `plan` was made from (qg_run_key.h); meaningful while plan != nullptr
    enum { NBUF = 6 + 16 };   // 0-5: host-layout A, B, C and packed A, B, C; behind them: the epilogue operands (2 per stage) or, on the
                              // root of a sharded call, the landing buffers of the other bands
    void* buf[NBUF] = {};
    size_t cap[NBUF] = {};
};
thread_local RunCache g_run;
// qgemul_run_sharded: one such cache per entry of the device list (slot i serves devices[i] of the calling thread's last list)
enum { QG_MAX_SHARDS = 16 };
thread_local RunCache g_shard[QG_MAX_SHARDS];
thread_local hipEvent_t g_shard_ev[QG_MAX_SHARDS] = {};
thread_local QRunKey g_want;   // the key of the request at hand (kept between calls: its APPROX tables are on the heap)
// What a thread has cached is released when the thread ends (worker threads that call Qgemul<>() and exit must not leak a stream
// and device buffers each).  For the main thread this runs inside exit() BEFORE any static object — HIP's included — is torn down.
std::atomic<bool> g_shutting_down{false};
void forget_caches();
struct RunCacheReaper {
    bool armed = false;
    ~RunCacheReaper()
    {
        if (!armed) return;
        int n = 0;
        // exit() has begun (atexit handlers run before static destruction, HIP's included) or the runtime no longer answers:
        // no HIP call from here, the driver reclaims the memory with the process
        if (g_shutting_down.load(std::memory_order_acquire) || hipGetDeviceCount(&n) != hipSuccess) { forget_caches(); return; }
        qgemul_run_release();
    }
};
thread_local RunCacheReaper g_reaper;
struct ShutdownHook {
    ShutdownHook() { atexit([] { g_shutting_down.store(true, std::memory_order_release); }); }
};
// every entry point that may fill a cache: this thread's reaper runs at its end, the hook is installed once per process
void arm_reaper()
{
    g_reaper.armed = true;
    static ShutdownHook hook;
}

int cache_buffer(RunCache& c, int i, size_t bytes, void** out)   // (the caller has made the cache's device current)
{
    if (bytes > c.cap[i]) {
        if (c.buf[i]) {
            hipStreamSynchronize(c.ctx->stream);
            hipFree(c.buf[i]);
            c.buf[i] = nullptr;
            c.cap[i] = 0;
        }
        const size_t want = bytes < 4096 ? 4096 : bytes;
        hipError_t e = hipMalloc(&c.buf[i], want);
        if (e != hipSuccess) { qg_set_last_hip((int)e); return QG_EHIP; }
        c.cap[i] = want;
    }
    *out = c.buf[i];
    return QG_OK;
}

void release_cache(RunCache& c)
{
    if (c.ctx) {
        DeviceScope scope(c.ctx->device);
        hipStreamSynchronize(c.ctx->stream);
        if (c.plan) qgemul_plan_destroy(c.plan);
        for (int i = 0; i < RunCache::NBUF; ++i) { if (c.buf[i]) hipFree(c.buf[i]); c.buf[i] = nullptr; c.cap[i] = 0; }
        qgemul_ctx_destroy(c.ctx);
    }
    c.plan = nullptr;
    c.ctx = nullptr;
    c.device = -2;
    c.key = QRunKey();
}

void forget_caches()
{
    auto forget = [](RunCache& c) {
        c.plan = nullptr;
        c.ctx = nullptr;
        c.device = -2;
        for (int i = 0; i < RunCache::NBUF; ++i) { c.buf[i] = nullptr; c.cap[i] = 0; }
    };
    forget(g_run);
    for (int i = 0; i < QG_MAX_SHARDS; ++i) { g_shard_ev[i] = nullptr; forget(g_shard[i]); }
}

// the cache's context serves `device` (< 0: whichever it is on); otherwise everything the cache holds goes and a new context comes
int cache_context(RunCache& c, int device)
{
    if (c.ctx && (device < 0 || device == c.device)) return QG_OK;
    release_cache(c);   // (only this cache: the others' contexts and plans stay warm)
    const int st = qgemul_ctx_create(device, &c.ctx);
    if (st != QG_OK) { c.ctx = nullptr; return st; }
    c.device = c.ctx->device;
    return QG_OK;
}

qgemul_opts resolve_opts(const qgemul_opts* o)
{
    qgemul_opts opts;
    memset(&opts, 0, sizeof opts);
    opts.device = -1;
    if (o) opts = *o;
    return opts;
}

// One single-device one-shot call.  batch == 0: the plain call (strides unused); batch > 0: `batch` members at constant strides.
// ev: the element-wise chain (nullptr: none) with its operands E; bep / strideE: a batched chain's shared and per-member operands.
struct RunRequest {
    const qgemul_desc* d;
    int64_t batch;
    const EpView* ev;
    const qgemul_batched_ep* bep;
    void* C;   // (with a chain: D)
    const void *A, *B;
    const void* const* E;
    int64_t strideC, strideA, strideB;
    const int64_t* strideE;
    qgemul_opts opts;
};

// the chain's operands: scalars into ea, tensors up to the device (slots 6 + 2k) and packed (slots 7 + 2k)
int stage_chain_operands(RunCache& c, const RunRequest& r, qgemul_ep_args& ea)
{
    const qgemul_desc* d = r.d;
    const EpView* ev = r.ev;
    const qgemul_epilogue* ep = ev->re;
    qgemul_plan* p = c.plan;
    hipStream_t s = c.ctx->stream;
    int st = QG_OK;
    memset(&ea, 0, sizeof ea);
    auto raw = [](const void* q, qfmt f) { return (1 + (int)f.I + (int)f.F) <= 32 ? (int64_t) * (const int32_t*)q : *(const int64_t*)q; };
    for (uint32_t k = 0; k < ep->n_stages; ++k) {
        const qgemul_ew_stage& sr = ep->stage[k];
        const qgemul_ew_stage* si = ev->im ? &ev->im->stage[k] : nullptr;
        const bool cplx = si && ev->e_cplx[k];
        if (sr.op == QG_EW_APPROX) continue;
        const bool t_re = sr.op != QG_EW_PASS && !sr.e_scalar, t_im = si && si->op != QG_EW_PASS && !si->e_scalar;
        if (!t_re && !t_im) {
            // scalar operand: one element ({re, im} for a complex one); a real scalar feeds both parts, except where the
            // imaginary part's stage takes the zero of the operand's type (real - complex, QuBLAS.h:3686)
            if (sr.op != QG_EW_PASS) ea.e_scalar[k] = raw(r.E[k], sr.e);
            if (si && si->op != QG_EW_PASS) {
                if (cplx) {
                    const qfmt f[2] = {sr.e, si->e};
                    ea.e_scalar_im[k] = raw((const char*)r.E[k] + qg_host_elem(f, 1).off[1], si->e);
                } else {
                    ea.e_scalar_im[k] = si->op == QG_EW_MUL ? raw(r.E[k], si->e) : 0;
                }
            }
            continue;
        }
        // tensor operand, tight: M x N elements; a batched chain's per-member operand: one every strideE[k] elements
        const qfmt f[2] = {t_re ? sr.e : si->e, si ? si->e : sr.e};
        const int64_t steps = r.batch > 0 && !r.bep->e_shared[k] ? (r.batch - 1) * r.strideE[k] : 0;
        const size_t bytesE = (size_t)(steps + d->M * d->N) * (size_t)qg_host_elem(f, cplx ? 1 : 0).size;
        void *dE, *pE;
        if ((st = cache_buffer(c, 6 + 2 * (int)k, bytesE, &dE)) || (st = cache_buffer(c, 7 + 2 * (int)k, (size_t)qgemul_packed_e_bytes(p, (int)k), &pE)))
            return st;
        if (hipMemcpyAsync(dE, r.E[k], bytesE, hipMemcpyHostToDevice, s) != hipSuccess) return QG_EHIP;
        if ((st = r.batch > 0 ? qgemul_pack_e_batched(p, (int)k, dE, 0, r.strideE[k], pE) : qgemul_pack_e(p, (int)k, dE, 0, pE))) return st;
        ea.e_packed[k] = pE;
        // (real - complex with a tensor operand: the imaginary part's stage has the scalar 0, set by the memset above)
    }
    return QG_OK;
}

int run_one_shot(const RunRequest& r)
{
    const qgemul_desc* d = r.d;
    const EpView* ev = r.ev;
    const qgemul_epilogue* ep = ev ? ev->re : nullptr;
    const int64_t batch = r.batch;
    qgemul_opts opts = r.opts;
    arm_reaper();
    RunCache& c = g_run;
    if (opts.device < 0 && c.ctx) {   // "current device": follow hipSetDevice calls the caller made between two calls
        int cur = c.device;
        if (hipGetDevice(&cur) == hipSuccess) opts.device = cur;
    }
    qg_run_key_set(g_want, *d, opts.flags, batch, ev, r.bep);
    const bool same_plan = c.plan && qg_run_key_equal(c.key, g_want) && (opts.device < 0 || opts.device == c.device);
    if (!same_plan) {
        // validate before touching the device so that descriptor errors are reported without a GPU
        qgemul_info info;
        const int st = batch > 0 ? classify_batched_view(d, batch, ev, r.bep, opts.flags, &info, nullptr) : classify_view(d, ev, opts.flags, &info);
        if (st != QG_OK) return st;
    }
    if (ep)
        for (uint32_t k = 0; k < ep->n_stages; ++k)
            if (ep->stage[k].op != QG_EW_APPROX && (!r.E || !r.E[k])) return QG_EINVAL;   // (an APPROX stage reads no operand)
    if (d->M == 0 || d->N == 0) return QG_OK;
    int st = QG_OK;
    const bool warm = c.ctx && (opts.device < 0 || opts.device == c.device);
    if ((st = cache_context(c, opts.device))) return st;
    if (warm) QG_HIP(hipSetDevice(c.device));
    if (!same_plan) {
        if (c.plan) { qgemul_plan_destroy(c.plan); c.plan = nullptr; }
        st = batch > 0 ? plan_create_batched_view(c.ctx, d, batch, ev, r.bep, opts.flags, &c.plan) : plan_create_view(c.ctx, d, ev, opts.flags, &c.plan);
        if (st != QG_OK) { c.plan = nullptr; return st; }
        c.key = g_want;
    }
    qgemul_plan* p = c.plan;
    void *dA, *dB, *dC, *pA, *pB, *pC;
    do {
        // host elements of one member (the plain call: of the whole operand) and, from there, of all of them
        const int64_t extA = qg_member_extent(*d, QG_OPERAND_A, opts.lda), extB = qg_member_extent(*d, QG_OPERAND_B, opts.ldb), extC = qg_member_extent(*d, QG_OPERAND_C, opts.ldc);
        if (extA < 1 || extB < 1 || extC < 1) { st = QG_EINVAL; break; }
        const int64_t more = batch > 0 ? batch - 1 : 0;
        const size_t bytesA = (size_t)(more * r.strideA + extA) * p->ha.size;
        const size_t bytesB = (size_t)(more * r.strideB + extB) * p->hb.size;
        const size_t bytesC = (size_t)(more * r.strideC + extC) * p->hc.size;
        if ((st = cache_buffer(c, 0, bytesA, &dA)) || (st = cache_buffer(c, 1, bytesB, &dB)) || (st = cache_buffer(c, 2, bytesC, &dC)) ||
            (st = cache_buffer(c, 3, (size_t)p->info.packed_bytes[0], &pA)) || (st = cache_buffer(c, 4, (size_t)p->info.packed_bytes[1], &pB)) ||
            (st = cache_buffer(c, 5, (size_t)p->info.packed_bytes[2], &pC)))
            break;
        hipStream_t s = c.ctx->stream;
        // everything below is queued on the context's stream; ONE synchronisation at the end (the source buffers are the
        // caller's and the call is synchronous, so they stay valid until then)
        if (hipMemcpyAsync(dA, r.A, bytesA, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(dB, r.B, bytesB, hipMemcpyHostToDevice, s) != hipSuccess) { st = QG_EHIP; break; }
        // the caller's C may have gaps between columns (ldc > M) and between members: those bytes stay as they are
        const bool gaps = (opts.ldc && opts.ldc != d->M) || (batch > 0 && r.strideC != d->M * d->N);
        if (gaps && hipMemcpyAsync(dC, r.C, bytesC, hipMemcpyHostToDevice, s) != hipSuccess) { st = QG_EHIP; break; }
        if (batch > 0) {
            if ((st = qgemul_pack_batched(p, QG_OPERAND_A, dA, opts.lda, r.strideA, pA)) || (st = qgemul_pack_batched(p, QG_OPERAND_B, dB, opts.ldb, r.strideB, pB))) break;
        } else {
            if ((st = qgemul_pack(p, QG_OPERAND_A, dA, opts.lda, pA)) || (st = qgemul_pack(p, QG_OPERAND_B, dB, opts.ldb, pB))) break;
        }
        if (!batch && !ep && stores_host_c(p)) {
            // the kernel's epilogue writes the reference layout: no packed C, no unpack pass
            if ((st = qgemul_execute_host_c(p, dC, opts.ldc, pA, pB))) break;
            if (hipMemcpyAsync(r.C, dC, bytesC, hipMemcpyDeviceToHost, s) != hipSuccess) { st = QG_EHIP; break; }
            break;
        }
        if (!ep) {
            if ((st = batch > 0 ? qgemul_execute_batched(p, pC, pA, pB) : qgemul_execute(p, pC, pA, pB))) break;
        } else {
            qgemul_ep_args ea;
            if ((st = stage_chain_operands(c, r, ea))) break;
            if ((st = batch > 0 ? qgemul_execute_batched_ep(p, pC, pA, pB, &ea) : qgemul_execute_ep(p, pC, pA, pB, &ea))) break;
        }
        if ((st = batch > 0 ? qgemul_unpack_c_batched(p, pC, dC, opts.ldc, r.strideC) : qgemul_unpack_c(p, pC, dC, opts.ldc))) break;
        if (hipMemcpyAsync(r.C, dC, bytesC, hipMemcpyDeviceToHost, s) != hipSuccess) { st = QG_EHIP; break; }
    } while (0);
    const hipError_t e = hipStreamSynchronize(c.ctx->stream);
    if (st == QG_OK && e != hipSuccess) { qg_set_last_hip((int)e); st = QG_EHIP; }
    return st;
}

// the plain call: QG_OPT_ALL_DEVICES goes to the sharded entry (without a chain: the element-wise chain runs on one device)
int run_view(const qgemul_desc* d, const EpView* ev, void* C, const void* A, const void* B, const void* const* E, const qgemul_opts* o)
{
    if (!d || !C || !A || !B) return QG_EINVAL;
    qgemul_opts opts = resolve_opts(o);
    if (opts.flags & QG_OPT_ALL_DEVICES) {
        if (ev) return QG_EUNSUPPORTED;
        if (d->is_complex && (d->cmul == QG_CMUL_REAL_A || d->cmul == QG_CMUL_REAL_B)) return QG_EUNSUPPORTED;   // (mixed real-complex: no sharded form)
        arm_reaper();
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return QG_ENOGPU;
        int list[QG_MAX_SHARDS];
        int n = 0;
        for (int i = 0; i < ndev && n < QG_MAX_SHARDS; ++i) list[n++] = i;
        opts.flags &= ~(uint32_t)QG_OPT_ALL_DEVICES;
        return qgemul_run_sharded(d, C, A, B, &opts, list, n);
    }
    const RunRequest r = {d, 0, ev, nullptr, C, A, B, E, 0, 0, 0, nullptr, opts};
    return run_one_shot(r);
}

// the batched calls' own checks, made before anything else: no sharded form, and every member inside its stride
int batched_args_ok(const qgemul_desc& d, const qgemul_opts& opts, int64_t strideC, int64_t strideA, int64_t strideB)
{
    if (opts.flags & QG_OPT_ALL_DEVICES) return QG_EUNSUPPORTED;   // (the sharded entry has no batched form)
    const int64_t extA = qg_member_extent(d, QG_OPERAND_A, opts.lda), extB = qg_member_extent(d, QG_OPERAND_B, opts.ldb), extC = qg_member_extent(d, QG_OPERAND_C, opts.ldc);
    if (extA < 1 || extB < 1 || extC < 1 || strideA < extA || strideB < extB || strideC < extC) return QG_EINVAL;
    return QG_OK;
}
} // namespace

extern "C" {

void qgemul_run_release(void)
{
    release_cache(g_run);
    for (int i = 0; i < QG_MAX_SHARDS; ++i) {
        if (g_shard_ev[i]) { hipEventDestroy(g_shard_ev[i]); g_shard_ev[i] = nullptr; }
        release_cache(g_shard[i]);
    }
}

int qgemul_run(const qgemul_desc* d, void* C, const void* A, const void* B, const qgemul_opts* o)
{
    return run_view(d, nullptr, C, A, B, nullptr, o);
}

int qgemul_run_ep(const qgemul_desc* d, const qgemul_epilogue* ep, void* C, const void* A, const void* B, const void* const* E,
                  const qgemul_opts* o)
{
    const EpView v = {ep, nullptr, nullptr};
    return run_view(d, ep ? &v : nullptr, C, A, B, E, o);
}

int qgemul_run_epx(const qgemul_desc* d, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], void* C, const void* A, const void* B,
                   const void* const* E, const qgemul_opts* o)
{
    if (!ep || !ax) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax};
    return run_view(d, &v, C, A, B, E, o);
}

int qgemul_run_epc(const qgemul_desc* d, const qgemul_epilogue_cplx* ep, void* C, const void* A, const void* B, const void* const* E,
                   const qgemul_opts* o)
{
    if (!ep) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex};
    return run_view(d, &v, C, A, B, E, o);
}

int qgemul_run_epcx(const qgemul_desc* d, const qgemul_epilogue_cplx* ep, const qgemul_cmul* const cx[QG_MAX_EW], void* C, const void* A,
                    const void* B, const void* const* E, const qgemul_opts* o)
{
    if (!ep || !cx) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex, nullptr, ep, cx};
    return run_view(d, &v, C, A, B, E, o);
}

// ---- batched Qgemul: `batch` GEMMs of one descriptor at constant strides (include/qgemul.h) ----
int qgemul_run_batched(const qgemul_desc* d, int64_t batch, void* C, const void* A, const void* B, int64_t strideC, int64_t strideA, int64_t strideB,
                       const qgemul_opts* o)
{
    if (!d || !C || !A || !B || batch < 1) return QG_EINVAL;
    const qgemul_opts opts = resolve_opts(o);
    if (const int st = batched_args_ok(*d, opts, strideC, strideA, strideB)) return st;
    const RunRequest r = {d, batch, nullptr, nullptr, C, A, B, nullptr, strideC, strideA, strideB, nullptr, opts};
    return run_one_shot(r);
}

// ... followed by a real element-wise chain: member b is Qgemul<...>(C_b, A_b, B_b), then the chain
int qgemul_run_batched_epx(const qgemul_desc* d, int64_t batch, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], void* D, const void* A,
                           const void* B, const void* const* E, int64_t strideD, int64_t strideA, int64_t strideB, const int64_t strideE[QG_MAX_EW],
                           const qgemul_opts* o)
{
    if (!d || !ep || !D || !A || !B || batch < 1 || ep->n_stages > QG_MAX_EW) return QG_EINVAL;
    const qgemul_opts opts = resolve_opts(o);
    if (const int st = batched_args_ok(*d, opts, strideD, strideA, strideB)) return st;
    const int64_t extE = qg_member_extent(*d, QG_OPERAND_C, 0);   // (stage operands are tight)
    qgemul_batched_ep bep;
    memset(&bep, 0, sizeof bep);
    for (uint32_t k = 0; k < ep->n_stages; ++k) {
        const qgemul_ew_stage& s = ep->stage[k];
        if (s.op == QG_EW_APPROX) continue;
        if (!E || !E[k]) return QG_EINVAL;
        if (s.e_scalar) continue;
        if (!strideE || (strideE[k] != 0 && strideE[k] < extE)) return QG_EINVAL;
        bep.e_shared[k] = strideE[k] == 0;
    }
    static const qgemul_approx* const no_ax[QG_MAX_EW] = {};   // (ax == nullptr: a chain without APPROX stages)
    const EpView v = {ep, nullptr, nullptr, ax ? ax : no_ax};
    const RunRequest r = {d, batch, &v, &bep, D, A, B, E, strideD, strideA, strideB, strideE, opts};
    return run_one_shot(r);
}

// ---- grouped Qgemul: `groups` GEMMs of different shapes (include/qgemul.h) ----
// The plan lives in the calling thread's one-plan cache, keyed on the WHOLE descriptor list: g_grp_key holds the list the cached
// plan was made from, and the cache's QRunKey marks the plan as a grouped one (batch = -groups: no plain or batched request has it).
namespace {
struct GrpKey {
    qgemul_desc* d = nullptr;
    int64_t n = 0;
    ~GrpKey() { delete[] d; }
};
thread_local GrpKey g_grp_key;
bool grp_key_equal(const qgemul_desc* d, int64_t groups)
{
    if (g_grp_key.n != groups || !g_grp_key.d) return false;
    for (int64_t g = 0; g < groups; ++g)
        if (!same_desc(g_grp_key.d[g], d[g])) return false;
    return true;
}
int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }
} // namespace

// ev: the group's one element-wise chain (nullptr: none; then gep, E and scalars are not read and C is C); with one, C is D, E[k][g] is
// member g's tight operand of tensor stage k (one element for a scalar stage that is not per member) and scalars[k] the per-member
// values of stage k.  The cache key holds the chain and, in the place of a batched chain's shared pattern, the per-member pattern
static int run_grouped_view(const qgemul_desc* d, int64_t groups, const EpView* ev, const qgemul_grouped_ep* gep, void* const* C, const void* const* A,
                            const void* const* B, const void* const* const* E, const int64_t* const* scalars, const int64_t* lda, const int64_t* ldb,
                            const int64_t* ldc, const qgemul_opts* o)
{
    if (!d || !C || !A || !B || groups < 1 || groups > 0x7fffffffll) return QG_EINVAL;
    qgemul_opts opts = resolve_opts(o);
    if (opts.flags & QG_OPT_ALL_DEVICES) return QG_EUNSUPPORTED;   // (the sharded entry has no grouped form)
    const qgemul_epilogue* ep = ev ? ev->re : nullptr;
    if (ep && ep->n_stages > QG_MAX_EW) return QG_EINVAL;
    qgemul_batched_ep pattern;
    memset(&pattern, 0, sizeof pattern);
    for (uint32_t k = 0; ep && k < ep->n_stages; ++k) {
        const qgemul_ew_stage& s = ep->stage[k];
        const bool per = gep && gep->scalar_per_member[k];
        pattern.e_shared[k] = per ? 1 : 0;
        if (s.op == QG_EW_APPROX) continue;
        if (per ? (!scalars || !scalars[k]) : (!E || !E[k])) return QG_EINVAL;
        for (int64_t g = 0; !per && g < groups; ++g)
            if (!(d[g].M == 0 || d[g].N == 0) && !E[k][s.e_scalar ? 0 : g]) return QG_EINVAL;
    }
    bool gaps = false;
    for (int64_t g = 0; g < groups; ++g) {
        if (d[g].M == 0 || d[g].N == 0) continue;
        if (!C[g] || !A[g] || !B[g]) return QG_EINVAL;
        if (qg_member_extent(d[g], QG_OPERAND_A, lda ? lda[g] : 0) < 1 || qg_member_extent(d[g], QG_OPERAND_B, ldb ? ldb[g] : 0) < 1 ||
            qg_member_extent(d[g], QG_OPERAND_C, ldc ? ldc[g] : 0) < 1)
            return QG_EINVAL;
        gaps |= ldc && ldc[g] && ldc[g] != d[g].M;
    }
    arm_reaper();
    RunCache& c = g_run;
    if (opts.device < 0 && c.ctx) {
        int cur = c.device;
        if (hipGetDevice(&cur) == hipSuccess) opts.device = cur;
    }
    qg_run_key_set(g_want, d[0], opts.flags, -groups, ev, ev ? &pattern : nullptr);
    const bool same_plan = c.plan && qg_run_key_equal(c.key, g_want) && grp_key_equal(d, groups) && (opts.device < 0 || opts.device == c.device);
    if (!same_plan) {   // validate before touching the device
        qgemul_info info;
        const int st = ev ? qgemul_classify_grouped_epx(d, groups, ep, ev->ax, gep, opts.flags, &info) : qgemul_classify_grouped(d, groups, opts.flags, &info);
        if (st != QG_OK) return st;
    }
    int st = QG_OK;
    const bool warm = c.ctx && (opts.device < 0 || opts.device == c.device);
    if ((st = cache_context(c, opts.device))) return st;
    if (warm) QG_HIP(hipSetDevice(c.device));
    if (!same_plan) {
        if (c.plan) { qgemul_plan_destroy(c.plan); c.plan = nullptr; }
        st = ev ? qgemul_plan_create_grouped_epx(c.ctx, d, groups, ep, ev->ax, gep, opts.flags, &c.plan) : qgemul_plan_create_grouped(c.ctx, d, groups, opts.flags, &c.plan);
        if (st != QG_OK) { c.plan = nullptr; return st; }
        c.key = g_want;
        delete[] g_grp_key.d;
        g_grp_key.d = new (std::nothrow) qgemul_desc[groups];
        g_grp_key.n = g_grp_key.d ? groups : 0;
        for (int64_t g = 0; g < g_grp_key.n; ++g) g_grp_key.d[g] = d[g];
    }
    qgemul_plan* p = c.plan;
    // the members' host-layout tensors back to back on the device, every start 256-byte aligned
    int64_t* off = new (std::nothrow) int64_t[3 * groups + 3];
    const void** dptr = new (std::nothrow) const void*[3 * groups];
    do {
        if (!off || !dptr) { st = QG_EINVAL; break; }
        int64_t tot[3] = {0, 0, 0};
        for (int64_t g = 0; g < groups; ++g) {
            const bool empty = d[g].M == 0 || d[g].N == 0;
            const int64_t ld[3] = {lda ? lda[g] : 0, ldb ? ldb[g] : 0, ldc ? ldc[g] : 0};
            for (int w = 0; w < 3; ++w) {
                off[3 * g + w] = tot[w];
                const qfmt* f = w == 0 ? d[g].a : w == 1 ? d[g].b : d[g].c;
                // (with a chain the third tensor is D: elements of the chain's destination format)
                const qfmt fd[2] = {ep ? ep->d : d[g].c[0], ep ? ep->d : d[g].c[1]};
                if (!empty) tot[w] += up256(qg_member_extent(d[g], w, ld[w]) * (int64_t)qg_host_elem(w == 2 ? fd : f, d[g].is_complex).size);
            }
        }
        void *dA, *dB, *dC, *pA, *pB, *pC;
        if ((st = cache_buffer(c, 0, (size_t)tot[0], &dA)) || (st = cache_buffer(c, 1, (size_t)tot[1], &dB)) || (st = cache_buffer(c, 2, (size_t)tot[2], &dC)) ||
            (st = cache_buffer(c, 3, (size_t)p->info.packed_bytes[0], &pA)) || (st = cache_buffer(c, 4, (size_t)p->info.packed_bytes[1], &pB)) ||
            (st = cache_buffer(c, 5, (size_t)p->info.packed_bytes[2], &pC)))
            break;
        hipStream_t s = c.ctx->stream;
        void* base[3] = {dA, dB, dC};
        auto bytes_of = [&](int64_t g, int w) {
            const int64_t ld = w == 0 ? (lda ? lda[g] : 0) : w == 1 ? (ldb ? ldb[g] : 0) : (ldc ? ldc[g] : 0);
            const qfmt fd[2] = {ep ? ep->d : d[g].c[0], ep ? ep->d : d[g].c[1]};
            const qfmt* f = w == 0 ? d[g].a : w == 1 ? d[g].b : fd;
            return (size_t)(qg_member_extent(d[g], w, ld) * (int64_t)qg_host_elem(f, d[g].is_complex).size);
        };
        for (int64_t g = 0; g < groups && st == QG_OK; ++g) {
            const bool empty = d[g].M == 0 || d[g].N == 0;
            for (int w = 0; w < 3; ++w) dptr[3 * g + w] = empty ? nullptr : (const char*)base[w] + off[3 * g + w];
            if (empty) continue;
            if (hipMemcpyAsync((void*)dptr[3 * g], A[g], bytes_of(g, 0), hipMemcpyHostToDevice, s) != hipSuccess ||
                hipMemcpyAsync((void*)dptr[3 * g + 1], B[g], bytes_of(g, 1), hipMemcpyHostToDevice, s) != hipSuccess ||
                (gaps && hipMemcpyAsync((void*)dptr[3 * g + 2], C[g], bytes_of(g, 2), hipMemcpyHostToDevice, s) != hipSuccess))   // (bytes between columns stay)
                st = QG_EHIP;
        }
        if (st != QG_OK) break;
        // (the pointer arrays of the entry points: one per operand)
        const void** pa_ = new (std::nothrow) const void*[3 * groups];
        if (!pa_) { st = QG_EINVAL; break; }
        for (int64_t g = 0; g < groups; ++g)
            for (int w = 0; w < 3; ++w) pa_[w * groups + g] = dptr[3 * g + w];
        // the chain's operands: scalars from the caller's one element or into the plan's table, tensors staged and packed member by member
        qgemul_ep_args ea;
        memset(&ea, 0, sizeof ea);
        auto raw = [](const void* q, qfmt f) { return (1 + (int)f.I + (int)f.F) <= 32 ? (int64_t) * (const int32_t*)q : *(const int64_t*)q; };
        const void** pe_ = ep ? new (std::nothrow) const void*[groups] : nullptr;
        if (ep && !pe_) st = QG_EINVAL;
        for (uint32_t k = 0; ep && k < ep->n_stages && st == QG_OK; ++k) {
            const qgemul_ew_stage& sk = ep->stage[k];
            if (sk.op == QG_EW_APPROX) continue;
            if (pattern.e_shared[k]) { st = qgemul_grouped_set_scalars(p, (int)k, scalars[k]); continue; }
            if (sk.e_scalar) { ea.e_scalar[k] = raw(E[k][0], sk.e); continue; }
            const qfmt fe[2] = {sk.e, sk.e};
            const int64_t eb = qg_host_elem(fe, 0).size;
            int64_t totE = 0;
            for (int64_t g = 0; g < groups; ++g) totE += d[g].M == 0 || d[g].N == 0 ? 0 : up256(d[g].M * d[g].N * eb);
            void *dE, *pE;
            if ((st = cache_buffer(c, 6 + 2 * (int)k, (size_t)totE, &dE)) || (st = cache_buffer(c, 7 + 2 * (int)k, (size_t)qgemul_packed_e_bytes(p, (int)k), &pE))) break;
            int64_t at = 0;
            for (int64_t g = 0; g < groups && st == QG_OK; ++g) {
                pe_[g] = nullptr;
                if (d[g].M == 0 || d[g].N == 0) continue;
                pe_[g] = (const char*)dE + at;
                if (hipMemcpyAsync((void*)pe_[g], E[k][g], (size_t)(d[g].M * d[g].N * eb), hipMemcpyHostToDevice, s) != hipSuccess) st = QG_EHIP;
                at += up256(d[g].M * d[g].N * eb);
            }
            if (st == QG_OK) st = qgemul_pack_e_grouped(p, (int)k, pe_, nullptr, pE);
            ea.e_packed[k] = pE;
        }
        delete[] pe_;
        if (st == QG_OK && !(st = qgemul_pack_grouped(p, QG_OPERAND_A, pa_, lda, pA)) && !(st = qgemul_pack_grouped(p, QG_OPERAND_B, pa_ + groups, ldb, pB)) &&
            !(st = ep ? qgemul_execute_grouped_ep(p, pC, pA, pB, &ea) : qgemul_execute_grouped(p, pC, pA, pB)))
            st = qgemul_unpack_c_grouped(p, pC, (void* const*)(pa_ + 2 * groups), ldc);
        delete[] pa_;
        for (int64_t g = 0; g < groups && st == QG_OK; ++g) {
            if (d[g].M == 0 || d[g].N == 0) continue;
            if (hipMemcpyAsync(C[g], dptr[3 * g + 2], bytes_of(g, 2), hipMemcpyDeviceToHost, s) != hipSuccess) st = QG_EHIP;
        }
    } while (0);
    const hipError_t e = hipStreamSynchronize(c.ctx->stream);
    delete[] off;
    delete[] dptr;
    if (st == QG_OK && e != hipSuccess) { qg_set_last_hip((int)e); st = QG_EHIP; }
    return st;
}

int qgemul_run_grouped(const qgemul_desc* d, int64_t groups, void* const* C, const void* const* A, const void* const* B, const int64_t* lda,
                       const int64_t* ldb, const int64_t* ldc, const qgemul_opts* o)
{
    return run_grouped_view(d, groups, nullptr, nullptr, C, A, B, nullptr, nullptr, lda, ldb, ldc, o);
}

// ... followed by ONE real element-wise chain with per-member scalars: member g is Qgemul<...>(C_g, A_g, B_g), then the chain
int qgemul_run_grouped_epx(const qgemul_desc* d, int64_t groups, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], const qgemul_grouped_ep* gep,
                           void* const* D, const void* const* A, const void* const* B, const void* const* const E[QG_MAX_EW],
                           const int64_t* const scalars[QG_MAX_EW], const int64_t* lda, const int64_t* ldb, const int64_t* ldd, const qgemul_opts* o)
{
    if (!ep) return QG_EINVAL;
    static const qgemul_approx* const no_ax[QG_MAX_EW] = {};   // (ax == nullptr: a chain without APPROX stages)
    const EpView v = {ep, nullptr, nullptr, ax ? ax : no_ax};
    return run_grouped_view(d, groups, &v, gep, D, A, B, E, scalars, lda, ldb, ldd, o);
}

// ---- several GPUs in one process: row bands of C, one per entry of the device list (include/qgemul.h) ----
// One host thread drives every device: all work is queued asynchronously on each device's own stream (H2D of the band of A
// and of B, pack, GEMM, peer copy of the packed C band to the root), the root's stream waits for each band's event, unpacks it
// into the one host-layout C and copies that back.  Bands are whole blocks of 256 rows (every packed row tile divides 256).
int qgemul_run_sharded(const qgemul_desc* d, void* C, const void* A, const void* B, const qgemul_opts* o, const int* devices, int n)
{
    if (!d || !C || !A || !B || !devices || n < 1 || n > QG_MAX_SHARDS) return QG_EINVAL;
    arm_reaper();
    qgemul_opts opts;
    memset(&opts, 0, sizeof opts);
    if (o) opts = *o;
    opts.flags &= ~(uint32_t)QG_OPT_ALL_DEVICES;
    {   // validate the whole problem before touching a device (a band of an unsupported descriptor is unsupported too)
        qgemul_info info;
        int st = qgemul_classify(d, opts.flags, &info);
        if (st != QG_OK) return st;
        // mixed real-complex descriptors have no sharded form yet (include/qgemul.h): one device serves them
        if (d->is_complex && (d->cmul == QG_CMUL_REAL_A || d->cmul == QG_CMUL_REAL_B)) return QG_EUNSUPPORTED;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return QG_ENOGPU;
    for (int i = 0; i < n; ++i)
        if (devices[i] < 0 || devices[i] >= ndev) return QG_EINVAL;
    if (d->M == 0 || d->N == 0) return QG_OK;
    const int64_t lda = opts.lda ? opts.lda : (d->transA ? d->K : d->M);
    const int64_t ldb = opts.ldb ? opts.ldb : d->K;
    const int64_t ldc = opts.ldc ? opts.ldc : d->M;
    if (lda < (d->transA ? d->K : d->M) || ldb < d->K || ldc < d->M) return QG_EINVAL;

    // contiguous bands of whole 256-row blocks, sizes differing by at most one block (qublas_amd/dist.py: row_partition)
    const int64_t ALIGN = 256, units = (d->M + ALIGN - 1) / ALIGN;
    int64_t row0[QG_MAX_SHARDS], rows[QG_MAX_SHARDS];
    {
        int64_t u0 = 0;
        for (int i = 0; i < n; ++i) {
            const int64_t u = units / n + (i < units % n ? 1 : 0);
            const int64_t r0 = u0 * ALIGN < d->M ? u0 * ALIGN : d->M, r1 = (u0 + u) * ALIGN < d->M ? (u0 + u) * ALIGN : d->M;
            row0[i] = r0;
            rows[i] = r1 - r0;
            u0 += u;
        }
    }
    int st = QG_OK;
    const int root = 0;   // devices[0] assembles C
    // contexts first: the root's is needed by every band
    for (int i = 0; i < n && st == QG_OK; ++i) {
        RunCache& c = g_shard[i];
        if ((st = cache_context(c, devices[i])) != QG_OK) break;
        if (!g_shard_ev[i]) {
            DeviceScope scope(c.device);
            if (hipEventCreateWithFlags(&g_shard_ev[i], hipEventDisableTiming) != hipSuccess) { g_shard_ev[i] = nullptr; st = QG_EHIP; }
        }
    }
    if (st != QG_OK) return st;
    RunCache& rc = g_shard[root];
    const qfmt* cf = d->c;
    const QHostElem hcel = qg_host_elem(cf, d->is_complex);
    const size_t bytesC = (size_t)((d->N - 1) * ldc + d->M) * hcel.size;
    void* dC = nullptr;   // host-layout C on the root
    {
        DeviceScope scope(rc.device);
        if ((st = cache_buffer(rc, 2, bytesC, &dC)) != QG_OK) return st;
        // the caller's C may have padding between columns (ldc > M): keep those bytes as they are
        if (ldc != d->M && hipMemcpyAsync(dC, C, bytesC, hipMemcpyHostToDevice, rc.ctx->stream) != hipSuccess) return QG_EHIP;
    }
    for (int i = 0; i < n && st == QG_OK; ++i) {
        if (rows[i] == 0) continue;
        RunCache& c = g_shard[i];
        DeviceScope scope(c.device);
        if (scope.err != hipSuccess) { st = QG_EHIP; break; }
        qgemul_desc bd = *d;
        bd.M = rows[i];
        qg_run_key_set(g_want, bd, opts.flags, 0, nullptr, nullptr);   // the band's plain plan
        if (!(c.plan && qg_run_key_equal(c.key, g_want))) {
            if (c.plan) { qgemul_plan_destroy(c.plan); c.plan = nullptr; }
            st = qgemul_plan_create(c.ctx, &bd, opts.flags, &c.plan);
            if (st != QG_OK) { c.plan = nullptr; break; }
            c.key = g_want;
        }
        qgemul_plan* p = c.plan;
        hipStream_t s = c.ctx->stream;
        const size_t ea = (size_t)p->ha.size, eb = (size_t)p->hb.size;
        // the band of A in host layout, tight on the device: A declared dim<M,K> (column-major) is strided in the band's rows,
        // A declared dim<K,M> (QgemulTransposedA) is one contiguous run of columns
        const size_t bytesA = d->transA ? (size_t)((rows[i] - 1) * lda + d->K) * ea : (size_t)rows[i] * (size_t)d->K * ea;
        const size_t bytesB = (size_t)((d->N - 1) * ldb + d->K) * eb;
        void *dA, *dB, *pA, *pB, *pC, *pCroot = nullptr;
        if ((st = cache_buffer(c, 0, bytesA, &dA)) || (st = cache_buffer(c, 1, bytesB, &dB)) ||
            (st = cache_buffer(c, 3, (size_t)p->info.packed_bytes[0], &pA)) || (st = cache_buffer(c, 4, (size_t)p->info.packed_bytes[1], &pB)) ||
            (st = cache_buffer(c, 5, (size_t)p->info.packed_bytes[2], &pC)))
            break;
        hipError_t he;
        int64_t band_lda;
        if (d->transA) {
            he = hipMemcpyAsync(dA, (const char*)A + (size_t)row0[i] * (size_t)lda * ea, bytesA, hipMemcpyHostToDevice, s);
            band_lda = lda;
        } else {
            he = hipMemcpy2DAsync(dA, (size_t)rows[i] * ea, (const char*)A + (size_t)row0[i] * ea, (size_t)lda * ea, (size_t)rows[i] * ea,
                                  (size_t)d->K, hipMemcpyHostToDevice, s);
            band_lda = rows[i];
        }
        if (he != hipSuccess || hipMemcpyAsync(dB, B, bytesB, hipMemcpyHostToDevice, s) != hipSuccess) { st = QG_EHIP; break; }
        if ((st = qgemul_pack(p, QG_OPERAND_A, dA, band_lda, pA)) || (st = qgemul_pack(p, QG_OPERAND_B, dB, ldb, pB)) ||
            (st = qgemul_execute(p, pC, pA, pB)))
            break;
        // the packed band goes to the root (a peer copy; the same device twice: a device-to-device copy), the root unpacks it
        if (i == root) {
            pCroot = pC;
        } else {
            // one landing buffer per band on the root: the slots behind the six fixed ones, grown on demand
            const int slot = 6 + (i - 1);
            if (slot >= RunCache::NBUF) { st = QG_EUNSUPPORTED; break; }
            {
                DeviceScope rscope(rc.device);
                if ((st = cache_buffer(rc, slot, (size_t)p->info.packed_bytes[2], &pCroot)) != QG_OK) break;
            }
            if (hipMemcpyPeerAsync(pCroot, rc.device, pC, c.device, (size_t)p->info.packed_bytes[2], s) != hipSuccess) { st = QG_EHIP; break; }
        }
        if (hipEventRecord(g_shard_ev[i], s) != hipSuccess) { st = QG_EHIP; break; }
        {
            DeviceScope rscope(rc.device);
            if (i != root && hipStreamWaitEvent(rc.ctx->stream, g_shard_ev[i], 0) != hipSuccess) { st = QG_EHIP; break; }
            QCGeom g = p->pc;          // the band's packed geometry, written at row offset row0 of the full C
            g.ldc = ldc;
            char* dst = (char*)dC + (size_t)row0[i] * hcel.size;
            if (qg_launch_unpack_c(g, pCroot, dst, rc.ctx->stream, (opts.flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0) != hipSuccess) { st = QG_EHIP; break; }
        }
    }
    if (st == QG_OK) {
        DeviceScope scope(rc.device);
        if (hipMemcpyAsync(C, dC, bytesC, hipMemcpyDeviceToHost, rc.ctx->stream) != hipSuccess) st = QG_EHIP;
    }
    // the call is synchronous: every stream drains before the caller's buffers may change (root last: it waits for the others)
    for (int i = n - 1; i >= 0; --i) {
        if (!g_shard[i].ctx) continue;
        DeviceScope scope(g_shard[i].device);
        const hipError_t e = hipStreamSynchronize(g_shard[i].ctx->stream);
        if (st == QG_OK && e != hipSuccess) { qg_set_last_hip((int)e); st = QG_EHIP; }
    }
    return st;
}

} // extern "C"
