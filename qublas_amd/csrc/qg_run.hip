// qg_run.hip — the one-shot calls of include/qgemul.h (qgemul_run*, qgemul_run_batched*, qgemul_run_grouped*, qgemul_run_sharded):
// host tensors in, host tensors out, one synchronous call.  The plain and batched entry points fill a RunRequest and go through
// run_one_shot, the grouped ones fill a GroupedRequest and go through run_grouped; both get the thread's cached plan from
// acquire_plan, their six operand buffers from cache_operand_buffers and their one synchronisation from finish.  The band loop of
// qgemul_run_sharded installs its plans with acquire_plan's second half, install_plan.
#include <atomic>
#include <memory>

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
thread_local QRunKey g_want;   // the key of the request at hand (kept between calls: its APPROX tables and descriptor list are on the heap)
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

// ---- the cache protocol, once ----
// the cache's plan is the one `want` names, or it goes and create(ctx, &plan) makes that one; a failed create leaves the cache without
// a plan.  (The caller has made the cache's device current.)
template <class Create>
int install_plan(RunCache& c, const QRunKey& want, Create create)
{
    if (c.plan && qg_run_key_equal(c.key, want)) return QG_OK;
    if (c.plan) { qgemul_plan_destroy(c.plan); c.plan = nullptr; }
    const int st = create(c.ctx, &c.plan);
    if (st != QG_OK) c.plan = nullptr; else c.key = want;
    return st;
}

// The calling thread's one-plan cache serves the request `want` on `device` (< 0: the caller's current one).  classify() is the
// request's host-only validation: it runs unless the cached plan is the request's, and its status is reported before a device is
// touched, so descriptor errors come out without a GPU.
template <class Classify, class Create>
int acquire_plan(RunCache& c, int device, const QRunKey& want, Classify classify, Create create)
{
    if (device < 0 && c.ctx) {   // "current device": follow hipSetDevice calls the caller made between two calls
        int cur = c.device;
        if (hipGetDevice(&cur) == hipSuccess) device = cur;
    }
    const bool warm = c.ctx && (device < 0 || device == c.device);
    int st = QG_OK;
    if (!(warm && c.plan && qg_run_key_equal(c.key, want)) && (st = classify())) return st;
    if ((st = cache_context(c, device))) return st;   // (another device: everything the cache held is gone)
    if (warm) QG_HIP(hipSetDevice(c.device));
    return install_plan(c, want, create);
}

// slots 0-5 of the cache: host-layout A, B and C (or D) of the given sizes, and the plan's packed A, B and C
struct OperandBuffers { void *dA, *dB, *dC, *pA, *pB, *pC; };
int cache_operand_buffers(RunCache& c, size_t bytesA, size_t bytesB, size_t bytesC, OperandBuffers& b)
{
    const int64_t* packed = c.plan->info.packed_bytes;
    int st;
    if ((st = cache_buffer(c, 0, bytesA, &b.dA)) || (st = cache_buffer(c, 1, bytesB, &b.dB)) || (st = cache_buffer(c, 2, bytesC, &b.dC)) ||
        (st = cache_buffer(c, 3, (size_t)packed[0], &b.pA)) || (st = cache_buffer(c, 4, (size_t)packed[1], &b.pB)) || (st = cache_buffer(c, 5, (size_t)packed[2], &b.pC)))
        return st;
    return QG_OK;
}

// Everything a call queues goes on the context's stream; ONE synchronisation ends the call, also after a failure mid-way (the source
// buffers are the caller's and the call is synchronous, so they stay valid until then).  st: what queueing returned; the first error counts
int finish(RunCache& c, int st)
{
    const hipError_t e = hipStreamSynchronize(c.ctx->stream);
    if (st == QG_OK && e != hipSuccess) { qg_set_last_hip((int)e); st = QG_EHIP; }
    return st;
}

// the raw value of a chain's scalar operand: one host element of format f
int64_t raw_scalar(const void* q, qfmt f) { return (1 + (int)f.I + (int)f.F) <= 32 ? (int64_t) * (const int32_t*)q : *(const int64_t*)q; }

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
    for (uint32_t k = 0; k < ep->n_stages; ++k) {
        const qgemul_ew_stage& sr = ep->stage[k];
        const qgemul_ew_stage* si = ev->im ? &ev->im->stage[k] : nullptr;
        const bool cplx = si && ev->e_cplx[k];
        if (sr.op == QG_EW_APPROX) continue;
        const bool t_re = sr.op != QG_EW_PASS && !sr.e_scalar, t_im = si && si->op != QG_EW_PASS && !si->e_scalar;
        if (!t_re && !t_im) {
            // scalar operand: one element ({re, im} for a complex one); a real scalar feeds both parts, except where the
            // imaginary part's stage takes the zero of the operand's type (real - complex, QuBLAS.h:3686)
            if (sr.op != QG_EW_PASS) ea.e_scalar[k] = raw_scalar(r.E[k], sr.e);
            if (si && si->op != QG_EW_PASS) {
                if (cplx) {
                    const qfmt f[2] = {sr.e, si->e};
                    ea.e_scalar_im[k] = raw_scalar((const char*)r.E[k] + qg_host_elem(f, 1).off[1], si->e);
                } else {
                    ea.e_scalar_im[k] = si->op == QG_EW_MUL ? raw_scalar(r.E[k], si->e) : 0;
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

// what run_one_shot queues on the cache's stream: upload, pack, the chain's operands, execute, unpack, download
int queue_one_shot(RunCache& c, const RunRequest& r)
{
    const qgemul_desc* d = r.d;
    const bool ep = r.ev != nullptr;
    const int64_t batch = r.batch;
    const qgemul_opts& opts = r.opts;
    qgemul_plan* p = c.plan;
    hipStream_t s = c.ctx->stream;
    int st = QG_OK;
    // host elements of one member (the plain call: of the whole operand) and, from there, of all of them
    const int64_t extA = qg_member_extent(*d, QG_OPERAND_A, opts.lda), extB = qg_member_extent(*d, QG_OPERAND_B, opts.ldb), extC = qg_member_extent(*d, QG_OPERAND_C, opts.ldc);
    if (extA < 1 || extB < 1 || extC < 1) return QG_EINVAL;
    const int64_t more = batch > 0 ? batch - 1 : 0;
    const size_t bytesA = (size_t)(more * r.strideA + extA) * p->ha.size;
    const size_t bytesB = (size_t)(more * r.strideB + extB) * p->hb.size;
    const size_t bytesC = (size_t)(more * r.strideC + extC) * p->hc.size;
    OperandBuffers b;
    if ((st = cache_operand_buffers(c, bytesA, bytesB, bytesC, b))) return st;
    if (hipMemcpyAsync(b.dA, r.A, bytesA, hipMemcpyHostToDevice, s) != hipSuccess || hipMemcpyAsync(b.dB, r.B, bytesB, hipMemcpyHostToDevice, s) != hipSuccess) return QG_EHIP;
    // the caller's C may have gaps between columns (ldc > M) and between members: those bytes stay as they are
    const bool gaps = (opts.ldc && opts.ldc != d->M) || (batch > 0 && r.strideC != d->M * d->N);
    if (gaps && hipMemcpyAsync(b.dC, r.C, bytesC, hipMemcpyHostToDevice, s) != hipSuccess) return QG_EHIP;
    if (batch > 0) {
        if ((st = qgemul_pack_batched(p, QG_OPERAND_A, b.dA, opts.lda, r.strideA, b.pA)) || (st = qgemul_pack_batched(p, QG_OPERAND_B, b.dB, opts.ldb, r.strideB, b.pB))) return st;
    } else {
        if ((st = qgemul_pack(p, QG_OPERAND_A, b.dA, opts.lda, b.pA)) || (st = qgemul_pack(p, QG_OPERAND_B, b.dB, opts.ldb, b.pB))) return st;
    }
    const bool host_c = !batch && !ep && stores_host_c(p);   // the kernel's epilogue writes the reference layout: no packed C, no unpack pass
    if (host_c) {
        if ((st = qgemul_execute_host_c(p, b.dC, opts.ldc, b.pA, b.pB))) return st;
    } else if (!ep) {
        if ((st = batch > 0 ? qgemul_execute_batched(p, b.pC, b.pA, b.pB) : qgemul_execute(p, b.pC, b.pA, b.pB))) return st;
    } else {
        qgemul_ep_args ea;
        if ((st = stage_chain_operands(c, r, ea))) return st;
        if ((st = batch > 0 ? qgemul_execute_batched_ep(p, b.pC, b.pA, b.pB, &ea) : qgemul_execute_ep(p, b.pC, b.pA, b.pB, &ea))) return st;
    }
    if (!host_c && (st = batch > 0 ? qgemul_unpack_c_batched(p, b.pC, b.dC, opts.ldc, r.strideC) : qgemul_unpack_c(p, b.pC, b.dC, opts.ldc))) return st;
    return hipMemcpyAsync(r.C, b.dC, bytesC, hipMemcpyDeviceToHost, s) == hipSuccess ? QG_OK : QG_EHIP;
}

int run_one_shot(const RunRequest& r)
{
    const qgemul_desc* d = r.d;
    const EpView* ev = r.ev;
    const int64_t batch = r.batch;
    const uint32_t flags = r.opts.flags;
    qgemul_info info;
    auto classify = [&] { return batch > 0 ? classify_batched_view(d, batch, ev, r.bep, flags, &info, nullptr) : classify_view(d, ev, flags, &info); };
    auto create = [&](qgemul_ctx* ctx, qgemul_plan** out) { return batch > 0 ? plan_create_batched_view(ctx, d, batch, ev, r.bep, flags, out) : plan_create_view(ctx, d, ev, flags, out); };
    // the last argument check, shared by every entry point: each stage's operand is there (a stage count the classifier will refuse is
    // read as far as the struct goes)
    for (uint32_t k = 0; ev && k < ev->re->n_stages && k < QG_MAX_EW; ++k)
        if (ev->re->stage[k].op != QG_EW_APPROX && (!r.E || !r.E[k])) return QG_EINVAL;   // (an APPROX stage reads no operand)
    if (d->M == 0 || d->N == 0) return classify();   // nothing to compute: the request's own status, no device touched
    arm_reaper();
    RunCache& c = g_run;
    qg_run_key_set(g_want, *d, flags, batch, ev, r.bep);
    if (const int st = acquire_plan(c, r.opts.device, g_want, classify, create)) return st;
    return finish(c, queue_one_shot(c, r));
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

// ---- the grouped one-shot call: `groups` GEMMs of different shapes, beside run_one_shot ----
// The plan lives in the calling thread's one-plan cache like every other one-shot plan; its key holds the WHOLE descriptor list.
// ev: the group's one element-wise chain (nullptr: none; then gep, E and scalars are not read and C is C); with one, C is D, E[k][g] is
// member g's tight operand of tensor stage k (one element for a scalar stage that is not per member) and scalars[k] the per-member
// values of stage k
struct GroupedRequest {
    const qgemul_desc* d;
    int64_t groups;
    const EpView* ev;
    const qgemul_grouped_ep* gep;
    void* const* C;   // (with a chain: D)
    const void* const *A, *const *B;
    const void* const* const* E;
    const int64_t* const* scalars;
    const int64_t *lda, *ldb, *ldc;
};
bool empty_member(const qgemul_desc& d) { return d.M == 0 || d.N == 0; }

// The host-only argument checks, made before anything else.  per: which scalar stages take a value per member, as 0 / 1 over the chain's
// stages (the cache key's and the layout's form of gep); gaps: a leading dimension of C leaves bytes between columns
int grouped_args_ok(const GroupedRequest& r, const qgemul_opts& opts, qgemul_grouped_ep& per, bool& gaps)
{
    const qgemul_desc* d = r.d;
    if (!d || !r.C || !r.A || !r.B || r.groups < 1 || r.groups > 0x7fffffffll) return QG_EINVAL;
    if (opts.flags & QG_OPT_ALL_DEVICES) return QG_EUNSUPPORTED;   // (the sharded entry has no grouped form)
    const qgemul_epilogue* ep = r.ev ? r.ev->re : nullptr;
    if (ep && ep->n_stages > QG_MAX_EW) return QG_EINVAL;
    memset(&per, 0, sizeof per);
    for (uint32_t k = 0; ep && k < ep->n_stages; ++k) {
        const qgemul_ew_stage& s = ep->stage[k];
        per.scalar_per_member[k] = r.gep && r.gep->scalar_per_member[k] ? 1 : 0;
        if (s.op == QG_EW_APPROX) continue;
        if (per.scalar_per_member[k] ? (!r.scalars || !r.scalars[k]) : (!r.E || !r.E[k])) return QG_EINVAL;
        for (int64_t g = 0; !per.scalar_per_member[k] && g < r.groups; ++g)
            if (!empty_member(d[g]) && !r.E[k][s.e_scalar ? 0 : g]) return QG_EINVAL;
    }
    gaps = false;
    for (int64_t g = 0; g < r.groups; ++g) {
        if (empty_member(d[g])) continue;   // (skipped everywhere: its pointers may be null)
        if (!r.C[g] || !r.A[g] || !r.B[g]) return QG_EINVAL;
        if (qg_member_extent(d[g], QG_OPERAND_A, r.lda ? r.lda[g] : 0) < 1 || qg_member_extent(d[g], QG_OPERAND_B, r.ldb ? r.ldb[g] : 0) < 1 ||
            qg_member_extent(d[g], QG_OPERAND_C, r.ldc ? r.ldc[g] : 0) < 1)
            return QG_EINVAL;
        gaps |= r.ldc && r.ldc[g] && r.ldc[g] != d[g].M;
    }
    return QG_OK;
}

// Where the members' host-layout tensors stand on the device: per tensor (A, B, C or D, then the chain's tensor operand of stage k at
// 3 + k) the members back to back in that tensor's buffer, every start 256-byte aligned.  Computed once; the uploads, the entry points'
// pointer arrays and the download read it.  An empty member, and every member of a stage without a tensor operand, has 0 bytes.
struct GroupedLayout {
    enum { NT = 3 + QG_MAX_EW };
    struct Span { int64_t off, bytes; };
    int64_t groups = 0;
    std::unique_ptr<Span[]> span;        // [t * groups + g]
    std::unique_ptr<const void*[]> ptr;  // [t * groups + g]: the member's device address once place() has the buffer (0 bytes: nullptr)
    int64_t total[NT] = {};
    const Span& at(int t, int64_t g) const { return span[t * groups + g]; }
    const void** ptrs(int t) const { return &ptr[t * groups]; }
    void place(int t, void* base)
    {
        for (int64_t g = 0; g < groups; ++g) ptr[t * groups + g] = at(t, g).bytes ? (const char*)base + at(t, g).off : nullptr;
    }
};
bool grouped_layout(GroupedLayout& L, const GroupedRequest& r, const qgemul_grouped_ep& per)
{
    const qgemul_epilogue* ep = r.ev ? r.ev->re : nullptr;
    const int64_t n = L.groups = r.groups;
    L.span.reset(new (std::nothrow) GroupedLayout::Span[GroupedLayout::NT * n]);
    L.ptr.reset(new (std::nothrow) const void*[GroupedLayout::NT * n]());
    if (!L.span || !L.ptr) return false;
    const int64_t* const ld[3] = {r.lda, r.ldb, r.ldc};
    for (int t = 0; t < GroupedLayout::NT; ++t) {
        const qgemul_ew_stage* sk = t >= 3 && ep && (uint32_t)(t - 3) < ep->n_stages ? &ep->stage[t - 3] : nullptr;
        const bool tensor = t < 3 || (sk && sk->op != QG_EW_APPROX && !sk->e_scalar && !per.scalar_per_member[t - 3]);
        for (int64_t g = 0; g < n; ++g) {
            const qgemul_desc& m = r.d[g];
            int64_t bytes = 0;
            if (tensor && !empty_member(m)) {
                if (t < 3) {
                    // (with a chain the third tensor is D: elements of the chain's destination format)
                    const qfmt fd[2] = {ep ? ep->d : m.c[0], ep ? ep->d : m.c[1]};
                    const qfmt* f = t == 0 ? m.a : t == 1 ? m.b : fd;
                    bytes = qg_member_extent(m, t, ld[t] ? ld[t][g] : 0) * (int64_t)qg_host_elem(f, m.is_complex).size;
                } else {
                    const qfmt fe[2] = {sk->e, sk->e};
                    bytes = m.M * m.N * (int64_t)qg_host_elem(fe, 0).size;   // (stage operands are tight)
                }
            }
            L.span[t * n + g] = {L.total[t], bytes};
            L.total[t] += (bytes + 255) / 256 * 256;
        }
    }
    return true;
}

// the grouped chain's operands: scalars from the caller's one element into ea or per member into the plan's table, tensors up to the
// device member by member (slots 6 + 2k) and packed (slots 7 + 2k)
int stage_grouped_chain_operands(RunCache& c, const GroupedRequest& r, const qgemul_grouped_ep& per, GroupedLayout& L, qgemul_ep_args& ea)
{
    const qgemul_epilogue* ep = r.ev->re;
    qgemul_plan* p = c.plan;
    hipStream_t s = c.ctx->stream;
    int st = QG_OK;
    memset(&ea, 0, sizeof ea);
    for (uint32_t k = 0; k < ep->n_stages; ++k) {
        const qgemul_ew_stage& sk = ep->stage[k];
        if (sk.op == QG_EW_APPROX) continue;
        if (per.scalar_per_member[k]) {
            if ((st = qgemul_grouped_set_scalars(p, (int)k, r.scalars[k]))) return st;
            continue;
        }
        if (sk.e_scalar) { ea.e_scalar[k] = raw_scalar(r.E[k][0], sk.e); continue; }
        const int t = 3 + (int)k;
        void *dE, *pE;
        if ((st = cache_buffer(c, 6 + 2 * (int)k, (size_t)L.total[t], &dE)) || (st = cache_buffer(c, 7 + 2 * (int)k, (size_t)qgemul_packed_e_bytes(p, (int)k), &pE))) return st;
        L.place(t, dE);
        for (int64_t g = 0; g < L.groups; ++g)
            if (L.at(t, g).bytes && hipMemcpyAsync((void*)L.ptrs(t)[g], r.E[k][g], (size_t)L.at(t, g).bytes, hipMemcpyHostToDevice, s) != hipSuccess) return QG_EHIP;
        if ((st = qgemul_pack_e_grouped(p, (int)k, L.ptrs(t), nullptr, pE))) return st;
        ea.e_packed[k] = pE;
    }
    return QG_OK;
}

// what run_grouped queues on the cache's stream: upload, the chain's operands, pack, execute, unpack, download
int queue_grouped(RunCache& c, const GroupedRequest& r, const qgemul_grouped_ep& per, bool gaps)
{
    qgemul_plan* p = c.plan;
    hipStream_t s = c.ctx->stream;
    int st = QG_OK;
    GroupedLayout L;
    if (!grouped_layout(L, r, per)) return QG_EINVAL;
    OperandBuffers b;
    if ((st = cache_operand_buffers(c, (size_t)L.total[0], (size_t)L.total[1], (size_t)L.total[2], b))) return st;
    void* const base[3] = {b.dA, b.dB, b.dC};
    const void* const* const host[3] = {r.A, r.B, (const void* const*)r.C};
    for (int t = 0; t < 3; ++t) {
        L.place(t, base[t]);
        if (t == 2 && !gaps) continue;   // C goes up only where a leading dimension leaves bytes between columns: they stay as they are
        for (int64_t g = 0; g < L.groups; ++g)
            if (L.at(t, g).bytes && hipMemcpyAsync((void*)L.ptrs(t)[g], host[t][g], (size_t)L.at(t, g).bytes, hipMemcpyHostToDevice, s) != hipSuccess) return QG_EHIP;
    }
    qgemul_ep_args ea;
    if (r.ev && (st = stage_grouped_chain_operands(c, r, per, L, ea))) return st;
    if ((st = qgemul_pack_grouped(p, QG_OPERAND_A, L.ptrs(0), r.lda, b.pA)) || (st = qgemul_pack_grouped(p, QG_OPERAND_B, L.ptrs(1), r.ldb, b.pB)) ||
        (st = r.ev ? qgemul_execute_grouped_ep(p, b.pC, b.pA, b.pB, &ea) : qgemul_execute_grouped(p, b.pC, b.pA, b.pB)) ||
        (st = qgemul_unpack_c_grouped(p, b.pC, (void* const*)L.ptrs(2), r.ldc)))
        return st;
    for (int64_t g = 0; g < L.groups; ++g)
        if (L.at(2, g).bytes && hipMemcpyAsync(r.C[g], L.ptrs(2)[g], (size_t)L.at(2, g).bytes, hipMemcpyDeviceToHost, s) != hipSuccess) return QG_EHIP;
    return QG_OK;
}

int run_grouped(const GroupedRequest& r, const qgemul_opts* o)
{
    const qgemul_opts opts = resolve_opts(o);
    qgemul_grouped_ep per;
    bool gaps;
    if (const int st = grouped_args_ok(r, opts, per, gaps)) return st;
    const EpView* ev = r.ev;
    qgemul_info info;
    auto classify = [&] { return ev ? qgemul_classify_grouped_epx(r.d, r.groups, ev->re, ev->ax, r.gep, opts.flags, &info) : qgemul_classify_grouped(r.d, r.groups, opts.flags, &info); };
    auto create = [&](qgemul_ctx* ctx, qgemul_plan** out) {
        return ev ? qgemul_plan_create_grouped_epx(ctx, r.d, r.groups, ev->re, ev->ax, r.gep, opts.flags, out) : qgemul_plan_create_grouped(ctx, r.d, r.groups, opts.flags, out);
    };
    arm_reaper();
    RunCache& c = g_run;
    qg_run_key_set_grouped(g_want, r.d, r.groups, opts.flags, ev, &per);
    if (const int st = acquire_plan(c, opts.device, g_want, classify, create)) return st;
    return finish(c, queue_grouped(c, r, per, gaps));
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
int qgemul_run_grouped(const qgemul_desc* d, int64_t groups, void* const* C, const void* const* A, const void* const* B, const int64_t* lda,
                       const int64_t* ldb, const int64_t* ldc, const qgemul_opts* o)
{
    const GroupedRequest r = {d, groups, nullptr, nullptr, C, A, B, nullptr, nullptr, lda, ldb, ldc};
    return run_grouped(r, o);
}

// ... followed by ONE real element-wise chain with per-member scalars: member g is Qgemul<...>(C_g, A_g, B_g), then the chain
int qgemul_run_grouped_epx(const qgemul_desc* d, int64_t groups, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], const qgemul_grouped_ep* gep,
                           void* const* D, const void* const* A, const void* const* B, const void* const* const E[QG_MAX_EW],
                           const int64_t* const scalars[QG_MAX_EW], const int64_t* lda, const int64_t* ldb, const int64_t* ldd, const qgemul_opts* o)
{
    if (!ep) return QG_EINVAL;
    static const qgemul_approx* const no_ax[QG_MAX_EW] = {};   // (ax == nullptr: a chain without APPROX stages)
    const EpView v = {ep, nullptr, nullptr, ax ? ax : no_ax};
    const GroupedRequest r = {d, groups, &v, gep, D, A, B, E, scalars, lda, ldb, ldd};
    return run_grouped(r, o);
}

// ---- several GPUs in one process: row bands of C, one per entry of the device list (include/qgemul.h) ----
// One host thread drives every device: all work is queued asynchronously on each device's own stream (H2D of the band of A
// and of B, pack, GEMM, peer copy of the packed C band to the root), the root's stream waits for each band's event, unpacks it
// into the one host-layout C and copies that back.  Bands are whole blocks of 256 rows (every packed row tile divides 256).
int qgemul_run_sharded(const qgemul_desc* d, void* C, const void* A, const void* B, const qgemul_opts* o, const int* devices, int n)
{
    if (!d || !C || !A || !B || !devices || n < 1 || n > QG_MAX_SHARDS) return QG_EINVAL;
    arm_reaper();
    qgemul_opts opts = resolve_opts(o);   // (opts.device is not read below: the device list names the devices)
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
        if ((st = install_plan(c, g_want, [&](qgemul_ctx* ctx, qgemul_plan** out) { return qgemul_plan_create(ctx, &bd, opts.flags, out); }))) break;
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
