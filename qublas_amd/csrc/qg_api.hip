// qg_api.hip — the C-ABI of include/qgemul.h: contexts, the entry points, plans and their device resources, packing, execution (the
// planner behind classification and plans: qg_geom.cpp; the one-shot calls: qg_run.hip).
//
// There is deliberately no CPU arithmetic path in this library: without a gfx950 device every
// compute entry point returns QG_ENOGPU.  (The CPU restatement lives in oracle/ and is test
// infrastructure only.)
#include "qg_api_int.h"

static thread_local int g_last_hip = 0;
int qg_last_hip() { return g_last_hip; }
void qg_set_last_hip(int e) { g_last_hip = e; }

struct HostC { void* C; int64_t ld; };   // execute_kernel: store the reference layout directly (kernels that can)

// composite plans: run `fn` on every (k-chunk, limb group) sub-operand of A or B — its view of the host tensor (the chunk's
// reduction indices), its packed geometry, its byte offset inside the packed operand
template <class F>
static hipError_t comp_for_each_sub(const qgemul_plan* p, int operand, const QOperandGeom& g, F fn)
{
    const QComposite& q = p->comp;
    const int w = operand == QG_OPERAND_A ? 0 : 1;
    const QPackedGeom& base = w ? p->pb : p->pa;
    for (int c = 0; c < q.nc; ++c)
        for (int gi = 0; gi < (w ? q.gb : q.ga); ++gi) {
            int64_t off = 0;
            const QPackedGeom sp = qg_comp_sub_geom(q, base, w, p->desc.K, c, gi, &off);
            QOperandGeom sg = g;
            sg.k0 = (int64_t)c * q.kc;
            sg.K = qg_comp_chunk_len(q, p->desc.K, c);
            if (hipError_t e = fn(sg, sp, off); e != hipSuccess) return e;
        }
    return hipSuccess;
}

// composite plan on a centred operand: its one row-sum array is zeroed before the sub-operands' packs add to it
static hipError_t comp_zero_rowsums(const qgemul_plan* p, int operand, void* packed_dev)
{
    const QPackedGeom& base = operand == QG_OPERAND_A ? p->pa : p->pb;
    if (!p->comp.on || !base.offs) return hipSuccess;
    return hipMemsetAsync((char*)packed_dev + base.rowsum_off, 0, (size_t)base.rows_p * 8, p->ctx->stream);
}

// centred operands (QPackedGeom::offs) and base-64 digit layouts (digit6): the limb kernels' epilogues take the bias back out with the
// row sums before the one round + overflow.  One bias per operand for everything the launch covers; K = 0: no corr (a grouped launch:
// its records carry K biasA biasB per member)
static void centre_args(QMfmaArgs& a, const QPackedGeom& ga, const QPackedGeom& gb, const void* packedA, const void* packedB, int64_t K)
{
    if (!ga.offs && !ga.digit6) return;
    a.rsA = (const int64_t*)((const char*)packedA + ga.rowsum_off);
    a.rsB = (const int64_t*)((const char*)packedB + gb.rowsum_off);
    a.biasA = ga.bias;
    a.biasB = gb.bias;
    a.corr = (int64_t)((uint64_t)K * (uint64_t)ga.bias * (uint64_t)gb.bias);
}

// QG_OPT_CHECK_RANGE: the packs between the two raise the context's flag on a raw value outside its declared format
static int range_check_begin(const qgemul_plan* p, int check)
{
    if (check) QG_HIP(hipMemsetAsync(p->ctx->flag_dev, 0, 4, p->ctx->stream));
    return QG_OK;
}
static int range_check_end(const qgemul_plan* p, int check)
{
    int flag = 0;
    if (!check) return QG_OK;
    QG_HIP(hipMemcpyAsync(&flag, p->ctx->flag_dev, 4, hipMemcpyDeviceToHost, p->ctx->stream));
    QG_HIP(hipStreamSynchronize(p->ctx->stream));
    return flag ? QG_ERANGE : QG_OK;
}

// plane mask of a packed multi-limb operand (QPackedGeom::trailer); nullptr: all planes
static const uint32_t* plane_mask(const void* packed, const QPackedGeom& g)
{
    return g.trailer ? (const uint32_t*)((const char*)packed + g.trailer) : nullptr;
}

// what every MFMA launch is given: operands of the geometries ga / gb, the result and its container, the kernel
static QMfmaArgs mfma_args(const QPackedGeom& ga, const QPackedGeom& gb, int variant, const void* A, const void* B, void* C, int cbytes)
{
    QMfmaArgs a;
    memset(&a, 0, sizeof a);
    a.A = (const int8_t*)A;
    a.B = (const int8_t*)B;
    a.C = C;
    a.Mp = ga.rows_p;
    a.Np = gb.rows_p;
    a.Kp = ga.K_p;
    a.cbytes = cbytes;
    a.variant = variant;
    a.maskA = plane_mask(A, ga);
    a.maskB = plane_mask(B, gb);
    return a;
}
// ... of a plan's own operands, with the one conversion into C's format and the centres of centred operands
static QMfmaArgs mfma_args(const qgemul_plan* p, const void* A, const void* B, void* C, int cbytes)
{
    QMfmaArgs a = mfma_args(p->pa, p->pb, p->variant, A, B, C, cbytes);
    a.to_c = p->an.lin.to_c[0];
    if (!p->comp.on) centre_args(a, p->pa, p->pb, A, B, p->desc.K);
    return a;
}

#ifdef QG_DIAG
static uint32_t* g_diag_stamps = nullptr;   // device buffer for in-kernel clock stamps (diagnostic build only)
extern "C" void qgemul_diag_set_stamps(void* dev) { g_diag_stamps = (uint32_t*)dev; }
#endif

// the mean time of `iters` calls of once() on the plan's stream, by HIP events, after `warmup` untimed ones
template <class F>
static int time_calls(qgemul_plan* p, int warmup, int iters, float* avg_ms, F once)
{
    QG_ON_DEVICE(p->ctx);
    hipStream_t st = p->ctx->stream;
    for (int i = 0; i < warmup; ++i)
        if (int s = once()) return s;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = QG_OK;
    float ms = 0;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, st);
    for (int i = 0; he == hipSuccess && rc == QG_OK && i < iters; ++i) rc = once();
    if (he == hipSuccess && rc == QG_OK) he = hipEventRecord(e1, st);
    if (he == hipSuccess && rc == QG_OK) he = hipEventSynchronize(e1);
    if (he == hipSuccess && rc == QG_OK) he = hipEventElapsedTime(&ms, e0, e1);
    if (e0) hipEventDestroy(e0);   // (released on every path)
    if (e1) hipEventDestroy(e1);
    if (he != hipSuccess) { g_last_hip = (int)he; return QG_EHIP; }
    if (rc != QG_OK) return rc;
    *avg_ms = ms / (float)iters;
    return QG_OK;
}

static bool fuses_epilogue(const qgemul_plan* p) { return qg_fuses_epilogue(p, p->flags, p->has_ax, p->has_cmul); }

extern "C" {

uint32_t qgemul_abi_version(void) { return QGEMUL_ABI_VERSION; }
int qgemul_last_hip_error(void) { return qg_last_hip(); }

const char* qgemul_strerror(int st)
{
    switch (st) {
    case QG_OK: return "ok";
    case QG_EINVAL: return "invalid descriptor or argument";
    case QG_EUNSUPPORTED: return "descriptor outside the engine's supported range";
    case QG_EHIP: return "HIP runtime error";
    case QG_ERCCL: return "RCCL error";
    case QG_ERANGE: return "input raw value outside its declared format";
    case QG_ENOGPU: return "no gfx950 device: the engine has no CPU fallback";
    default: return "unknown status";
    }
}

int qgemul_classify(const qgemul_desc* d, uint32_t opt_flags, qgemul_info* out) { return qgemul_classify_ep(d, nullptr, opt_flags, out); }

int classify_view(const qgemul_desc* d, const EpView* ev, uint32_t opt_flags, qgemul_info* out)
{
    if (!d || !out) return QG_EINVAL;
    QPlanGeom* g = new (std::nothrow) QPlanGeom();
    if (!g) return QG_EINVAL;
    const int st = qg_plan_geometry(d, opt_flags, ev, 0, g, nullptr, nullptr);
    *out = g->info;
    delete g;
    return st;
}

int qgemul_classify_ep(const qgemul_desc* d, const qgemul_epilogue* ep, uint32_t opt_flags, qgemul_info* out)
{
    const EpView v = {ep, nullptr, nullptr};
    return classify_view(d, ep ? &v : nullptr, opt_flags, out);
}

int qgemul_classify_epx(const qgemul_desc* d, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], uint32_t opt_flags, qgemul_info* out)
{
    if (!ep || !ax) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax};
    return classify_view(d, &v, opt_flags, out);
}

int qgemul_approx_plan_form(const qgemul_desc* d, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], qgemul_approx_form* out)
{
    if (!d || !ep || !ax || !out) return QG_EINVAL;
    memset(out, 0, sizeof *out);
    if (d->is_complex) return QG_EINVAL;
    QApproxTable* axt = new (std::nothrow) QApproxTable[QG_MAX_EW];
    if (!axt) return QG_EINVAL;
    QEpTable t;
    int bits = 0;
    const int st = qg_analyze_epx(d->c[0], ep, ax, &t, axt, &bits, nullptr, 0);
    if (st == QG_OK) {
        out->bits32 = t.bits32;
        out->max_bits = bits;
        for (int k = 0; k < QG_MAX_EW; ++k) {
            const bool on = k < t.n && t.st[k].op == QG_EW_APPROX;
            out->uniform[k] = on ? axt[k].uniform : -1;
            for (int g = 0; on && g < QG_MAX_SEG; ++g) out->threshold[k][g] = axt[k].thr[g];
        }
    }
    delete[] axt;
    return st;
}

size_t qgemul_sizeof(int which)
{
    switch (which) {
    case QG_SIZEOF_QFMT: return sizeof(qfmt);
    case QG_SIZEOF_DESC: return sizeof(qgemul_desc);
    case QG_SIZEOF_OPTS: return sizeof(qgemul_opts);
    case QG_SIZEOF_INFO: return sizeof(qgemul_info);
    case QG_SIZEOF_EW_STAGE: return sizeof(qgemul_ew_stage);
    case QG_SIZEOF_EPILOGUE: return sizeof(qgemul_epilogue);
    case QG_SIZEOF_EP_ARGS: return sizeof(qgemul_ep_args);
    case QG_SIZEOF_EPILOGUE_CPLX: return sizeof(qgemul_epilogue_cplx);
    case QG_SIZEOF_APPROX_SEG: return sizeof(qgemul_approx_seg);
    case QG_SIZEOF_APPROX: return sizeof(qgemul_approx);
    case QG_SIZEOF_CMUL: return sizeof(qgemul_cmul);
    case QG_SIZEOF_GROUPED_MEMBER: return sizeof(qgemul_grouped_member);
    case QG_SIZEOF_GROUPED_EP: return sizeof(qgemul_grouped_ep);
    default: return 0;
    }
}

int qgemul_classify_epc(const qgemul_desc* d, const qgemul_epilogue_cplx* ep, uint32_t opt_flags, qgemul_info* out)
{
    if (!ep) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex};
    return classify_view(d, &v, opt_flags, out);
}

int qgemul_classify_epcx(const qgemul_desc* d, const qgemul_epilogue_cplx* ep, const qgemul_cmul* const cx[QG_MAX_EW], uint32_t opt_flags, qgemul_info* out)
{
    if (!ep || !cx) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex, nullptr, ep, cx};
    return classify_view(d, &v, opt_flags, out);
}

int qgemul_cmul_plan_form(const qgemul_desc* d, const qgemul_epilogue_cplx* ep, const qgemul_cmul* const cx[QG_MAX_EW], qgemul_cmul_form* out)
{
    if (!d || !ep || !cx || !out) return QG_EINVAL;
    memset(out, 0, sizeof *out);
    if (!d->is_complex) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex, nullptr, ep, cx};
    if (!qg_view_has_cmul(&v)) {
        for (int k = 0; k < QG_MAX_EW; ++k)
            if (cx[k]) return QG_EINVAL;
        return QG_OK;
    }
    QEpTable t[2];
    int bits = 0;
    const int st = qg_analyze_epcx(d->c, ep, cx, t, nullptr, &bits, nullptr, 0);
    if (st == QG_OK) {
        out->has_cmul = 1;
        out->bits32 = t[0].bits32;
        out->max_bits = bits;
    }
    return st;
}

int qgemul_ctx_create(int device, qgemul_ctx** out)
{
    if (!out) return QG_EINVAL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return QG_ENOGPU;
    if (device < 0) QG_HIP(hipGetDevice(&device));
    if (device >= n) return QG_EINVAL;
    DeviceScope scope(device);   // the caller's current device is restored on return
    QG_HIP(scope.err);
    hipDeviceProp_t prop;
    QG_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return QG_ENOGPU; // kernels exist for gfx950 only
    qgemul_ctx* c = (qgemul_ctx*)calloc(1, sizeof *c);
    if (!c) return QG_EINVAL;
    c->device = device;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { free(c); return QG_EHIP; }
    if (hipMalloc((void**)&c->flag_dev, 64) != hipSuccess) { hipStreamDestroy(c->stream); free(c); return QG_EHIP; }
    hipMemsetAsync(c->flag_dev, 0, 64, c->stream);
    *out = c;
    return QG_OK;
}

void qgemul_ctx_destroy(qgemul_ctx* c)
{
    if (!c) return;
    DeviceScope scope(c->device);
    hipStreamSynchronize(c->stream);
    hipFree(c->flag_dev);
    hipStreamDestroy(c->stream);
    free(c);
}

int qgemul_ctx_sync(qgemul_ctx* c)
{
    if (!c) return QG_EINVAL;
    QG_ON_DEVICE(c);
    QG_HIP(hipStreamSynchronize(c->stream));
    return QG_OK;
}

void* qgemul_ctx_stream(qgemul_ctx* c) { return c ? (void*)c->stream : nullptr; }
int qgemul_ctx_device(const qgemul_ctx* c) { return c ? c->device : -1; }

int qgemul_dev_alloc(qgemul_ctx* c, size_t bytes, void** out)
{
    if (!c || !out) return QG_EINVAL;
    QG_ON_DEVICE(c);
    QG_HIP(hipMalloc(out, bytes ? bytes : 16));
    return QG_OK;
}
int qgemul_dev_free(qgemul_ctx* c, void* p)
{
    if (!c) return QG_EINVAL;
    QG_ON_DEVICE(c);
    QG_HIP(hipStreamSynchronize(c->stream));
    QG_HIP(hipFree(p));
    return QG_OK;
}
int qgemul_memcpy_h2d(qgemul_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return QG_EINVAL;
    if (!bytes) return QG_OK;
    QG_ON_DEVICE(c);
    QG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
    QG_HIP(hipStreamSynchronize(c->stream));
    return QG_OK;
}
int qgemul_memcpy_d2h(qgemul_ctx* c, void* dst, const void* src, size_t bytes)
{
    if (!c) return QG_EINVAL;
    if (!bytes) return QG_OK;
    QG_ON_DEVICE(c);
    QG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    QG_HIP(hipStreamSynchronize(c->stream));
    return QG_OK;
}

int qgemul_plan_create(qgemul_ctx* c, const qgemul_desc* d, uint32_t opt_flags, qgemul_plan** out)
{
    return qgemul_plan_create_ep(c, d, nullptr, opt_flags, out);
}

int qgemul_plan_create_ep(qgemul_ctx* c, const qgemul_desc* d, const qgemul_epilogue* ep, uint32_t opt_flags, qgemul_plan** out)
{
    const EpView v = {ep, nullptr, nullptr};
    return plan_create_view(c, d, ep ? &v : nullptr, opt_flags, out);
}

int qgemul_plan_create_epx(qgemul_ctx* c, const qgemul_desc* d, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], uint32_t opt_flags,
                           qgemul_plan** out)
{
    if (!ep || !ax) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax};
    return plan_create_view(c, d, &v, opt_flags, out);
}

int qgemul_plan_approx_uniform(const qgemul_plan* p) { return p && p->has_ax ? p->ax_uniform : -1; }

int qgemul_plan_create_epc(qgemul_ctx* c, const qgemul_desc* d, const qgemul_epilogue_cplx* ep, uint32_t opt_flags, qgemul_plan** out)
{
    if (!ep) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex};
    return plan_create_view(c, d, &v, opt_flags, out);
}

int qgemul_plan_create_epcx(qgemul_ctx* c, const qgemul_desc* d, const qgemul_epilogue_cplx* ep, const qgemul_cmul* const cx[QG_MAX_EW],
                            uint32_t opt_flags, qgemul_plan** out)
{
    if (!ep || !cx) return QG_EINVAL;
    const EpView v = {&ep->part[0], &ep->part[1], ep->e_complex, nullptr, ep, cx};
    return plan_create_view(c, d, &v, opt_flags, out);
}

int plan_create_view(qgemul_ctx* c, const qgemul_desc* d, const EpView* ev, uint32_t opt_flags, qgemul_plan** out, int64_t batch)   // batch > 0: the member of a batched plan
{
    if (!c || !d || !out) return QG_EINVAL;
    qgemul_plan* p = new (std::nothrow) qgemul_plan;
    if (!p) return QG_EINVAL;
    memset(p, 0, sizeof *p);
    p->ctx = c;
    p->desc = *d;
    p->flags = opt_flags;
    if (ev) {
        p->has_ep = 1;
        p->ep = *ev->re;
        if (ev->im) {
            p->ep_cplx = 1;
            p->ep_im = *ev->im;
            memcpy(p->e_cplx, ev->e_cplx, sizeof p->e_cplx);
        }
        for (int k = 0; ev->ax && k < QG_MAX_EW; ++k) p->has_ax |= ev->ax[k] != nullptr;
        p->has_cmul = qg_view_has_cmul(ev) ? 1 : 0;
        for (int k = 0; p->has_cmul && k < QG_MAX_EW; ++k)
            if (ev->cx[k]) p->cx[k] = *ev->cx[k];
    }
    QCmulStage cmt[QG_MAX_EW];
    QApproxTable* axt = p->has_ax ? new (std::nothrow) QApproxTable[QG_MAX_EW] : nullptr;
    if (p->has_ax && !axt) { delete p; return QG_EINVAL; }
    struct AxtGuard { QApproxTable* t; ~AxtGuard() { delete[] t; } } axt_guard = {axt};
    int st = qg_plan_geometry(d, opt_flags, ev, batch, p, axt, p->has_cmul ? cmt : nullptr);
    if (st != QG_OK) { delete p; return st; }
    p->tc = qg_tree_choice(&p->an, d, opt_flags, true);
    // from here on the plan may own device memory: every failure leaves through qgemul_plan_destroy, which frees whatever there is
    const auto fail = [p] { qgemul_plan_destroy(p); return QG_EHIP; };
    DeviceScope scope(c->device);
    if (scope.err != hipSuccess || hipMalloc((void**)&p->dev_table, sizeof(QTreeTable)) != hipSuccess) return fail();
    if (hipMemcpyAsync(p->dev_table, &p->an.tree, sizeof(QTreeTable), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail();
    if (p->info.kernel == QG_KERNEL_MFMA_CPLX || p->info.kernel == QG_KERNEL_MFMA_RC) {   // (a mixed plan's real operand has one part)
        const size_t ws = (size_t)((d->cmul == QG_CMUL_REAL_A ? 1 : 2) * p->pa.rows_p) * (size_t)((d->cmul == QG_CMUL_REAL_B ? 1 : 2) * p->pb.rows_p) * sizeof(int64_t);
        if (hipMalloc((void**)&p->workspace, ws) != hipSuccess) return fail();
    }
    if (qg_wide_epilogue(p) && hipMalloc((void**)&p->wide_ws, (size_t)(p->pc_c.Mp * p->pc_c.Np) * sizeof(int32_t)) != hipSuccess) return fail();
    if (p->comp.on) {
        const size_t n = (size_t)p->pa.rows_p * (size_t)p->pb.rows_p;
        const size_t sl = n * (size_t)(p->comp.ga * p->comp.gb) * (size_t)p->comp.slab_bytes;
        const size_t ac = p->comp.nc > 1 ? n * (p->comp.wide ? 16 : 8) : 0;
        if (hipMalloc(&p->comp_slabs, sl ? sl : 16) != hipSuccess || (ac && hipMalloc(&p->comp_acc, ac) != hipSuccess)) return fail();
    }
    if (p->has_ep && !fuses_epilogue(p)) {
        // the tree kernels store C; the chain then runs as a pass over it
        const size_t cb = (size_t)(p->pc_c.parts * p->pc_c.Mp * p->pc_c.Np) * (size_t)p->pc_c.cbytes;
        if (hipMalloc(&p->cwork, cb ? cb : 16) != hipSuccess) return fail();
    }
    if (p->has_ax) {
        // the plan's copy of the tables, pre-resolved: one device buffer per APPROX stage
        p->ax_uniform = 1;
        bool ok = true;
        for (int k = 0; k < p->ept.n && ok; ++k) {
            if (p->ept.st[k].op != QG_EW_APPROX) continue;
            p->ax_uniform &= axt[k].uniform;
            ok = hipMalloc((void**)&p->ax_dev[k], sizeof(QApproxTable)) == hipSuccess &&
                 hipMemcpyAsync(p->ax_dev[k], &axt[k], sizeof(QApproxTable), hipMemcpyHostToDevice, c->stream) == hipSuccess;
        }
        if (!ok || hipStreamSynchronize(c->stream) != hipSuccess) return fail();   // (the tables are host temporaries: copied before they go)
    }
    if (p->has_cmul) {
        // the pre-resolved records of the CMUL stages: one device buffer (host temporaries: copied before they go)
        if (hipMalloc((void**)&p->cm_dev, sizeof cmt) != hipSuccess ||
            hipMemcpyAsync(p->cm_dev, cmt, sizeof cmt, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
            return fail();
    }
    *out = p;
    return QG_OK;
}

void qgemul_plan_destroy(qgemul_plan* p)
{
    if (!p) return;
    if (p->member) qgemul_plan_destroy(p->member);   // (a batched plan: its member owns the device resources)
    if (p->grp) {                                      // (a grouped plan: the distinct descriptors' plans do)
        for (int64_t u = 0; u < p->grp->n_uniq; ++u)
            if (p->grp->up[u]) qgemul_plan_destroy(p->grp->up[u]);
    }
    DeviceScope scope(p->ctx->device);
    hipStreamSynchronize(p->ctx->stream);
    if (p->grp) {
        hipFree(p->grp->tiles_dev);
        hipFree(p->grp->tile_member_dev);
        hipFree(p->grp->cwork_dev);
        for (int k = 0; k < QG_MAX_EW; ++k) hipFree(p->grp->scal_dev[k]);
    }
    delete p->grp;
    hipFree(p->dev_table);
    hipFree(p->workspace);
    hipFree(p->stack_work);
    hipFree(p->cwork);
    hipFree(p->wide_ws);
    hipFree(p->hostc_pc);
    hipFree(p->comp_slabs);
    hipFree(p->comp_acc);
    for (int k = 0; k < QG_MAX_EW; ++k) hipFree(p->ax_dev[k]);
    hipFree(p->cm_dev);
    delete p;
}

int qgemul_plan_info(const qgemul_plan* p, qgemul_info* out)
{
    if (!p || !out) return QG_EINVAL;
    *out = p->info;
    return QG_OK;
}

static QOperandGeom operand_geom(const qgemul_plan* p, int operand, int64_t ld)
{
    const qgemul_desc& d = p->desc;
    QOperandGeom g;
    memset(&g, 0, sizeof g);
    const QHostElem& h = operand == QG_OPERAND_A ? p->ha : p->hb;
    const qfmt* f = operand == QG_OPERAND_A ? d.a : d.b;
    g.K = d.K;
    g.parts = d.is_complex && d.cmul != (operand == QG_OPERAND_A ? QG_CMUL_REAL_A : QG_CMUL_REAL_B) ? 2 : 1;   // (a mixed descriptor's real operand: plain words)
    g.elem_bytes = h.size;
    for (int q = 0; q < 2; ++q) {
        g.off[q] = h.off[q];
        g.sb[q] = h.sb[q];
        g.W[q] = (int)f[q].I + (int)f[q].F;
        g.S[q] = f[q].S;
        g.F[q] = f[q].F;
        g.Q[q] = f[q].Q;
        g.O[q] = f[q].O;
    }
    if (operand == QG_OPERAND_A) {
        g.rows = d.M;
        if (d.transA) { g.rs = ld ? ld : d.K; g.ks = 1; }   // A declared dim<K,M>: (i,k) at k + i*ld
        else { g.rs = 1; g.ks = ld ? ld : d.M; }            // A declared dim<M,K>: (i,k) at i + k*ld
    } else {
        g.rows = d.N;
        g.rs = ld ? ld : d.K;                                // B declared dim<K,N>: (k,j) at k + j*ld
        g.ks = 1;
    }
    return g;
}

int qgemul_pack(qgemul_plan* p, int operand, const void* src_dev, int64_t ld, void* packed_dev)
{
    if (!p || !src_dev || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    QG_ON_DEVICE(p->ctx);
    QOperandGeom g = operand_geom(p, operand, ld);
    const QPackedGeom& pg = operand == QG_OPERAND_A ? p->pa : p->pb;
    const int check = (p->flags & QG_OPT_CHECK_RANGE) ? 1 : 0;
    if (const int st = range_check_begin(p, check); st != QG_OK) return st;
    if (p->comp.on) {
        QG_HIP(comp_zero_rowsums(p, operand, packed_dev));
        QG_HIP(comp_for_each_sub(p, operand, g, [&](const QOperandGeom& sg, const QPackedGeom& sp, int64_t off) {
            return qg_launch_pack(sg, sp, src_dev, (char*)packed_dev + off, check, p->ctx->flag_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0);
        }));
    } else
    QG_HIP(qg_launch_pack(g, pg, src_dev, packed_dev, check, p->ctx->flag_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    return range_check_end(p, check);
}

int qgemul_pack_f64(qgemul_plan* p, int operand, const double* src_dev, int64_t ld, void* packed_dev)
{
    if (!p || !src_dev || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (!(p->flags & QG_OPT_ARITHMETIC_CONV)) {
        // Qu_s(double) with QuMode<RND::CONV>: the reference's result is an artefact of its multi-word CONV branch
        // (QuBLAS.h:2137-2156 on ArbiInt<2400>); silently returning the arithmetic answer would break bit-exactness
        const qfmt* f = operand == QG_OPERAND_A ? p->desc.a : p->desc.b;
        const int real_operand = p->desc.cmul == (operand == QG_OPERAND_A ? QG_CMUL_REAL_A : QG_CMUL_REAL_B);
        for (int q = 0; q < (p->desc.is_complex && !real_operand ? 2 : 1); ++q)
            if (f[q].Q == QG_RND_CONV) return QG_EUNSUPPORTED;
    }
    QG_ON_DEVICE(p->ctx);
    QOperandGeom g = operand_geom(p, operand, ld);
    const QPackedGeom& pg = operand == QG_OPERAND_A ? p->pa : p->pb;
    if (p->comp.on) {
        QG_HIP(comp_zero_rowsums(p, operand, packed_dev));
        QG_HIP(comp_for_each_sub(p, operand, g, [&](const QOperandGeom& sg, const QPackedGeom& sp, int64_t off) {
            return qg_launch_pack_f64(sg, sp, src_dev, (char*)packed_dev + off, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0);
        }));
        return QG_OK;
    }
    QG_HIP(qg_launch_pack_f64(g, pg, src_dev, packed_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    return QG_OK;
}

int qgemul_fill_packed(qgemul_plan* p, int operand, uint64_t seed, int dist, void* packed_dev)
{
    if (!p || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    QG_ON_DEVICE(p->ctx);
    QOperandGeom g = operand_geom(p, operand, 0);
    const QPackedGeom& pg = operand == QG_OPERAND_A ? p->pa : p->pb;
    if (p->comp.on) {
        QG_HIP(comp_zero_rowsums(p, operand, packed_dev));
        QG_HIP(comp_for_each_sub(p, operand, g, [&](const QOperandGeom& sg, const QPackedGeom& sp, int64_t off) {
            return qg_launch_fill(sg, sp, seed, dist, (char*)packed_dev + off, p->ctx->stream);
        }));
        return QG_OK;
    }
    QG_HIP(qg_launch_fill(g, pg, seed, dist, packed_dev, p->ctx->stream));
    return QG_OK;
}

int qgemul_unpack_c(qgemul_plan* p, const void* packed_dev, void* dst_dev, int64_t ld)
{
    if (!p || !packed_dev || !dst_dev) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    QG_ON_DEVICE(p->ctx);
    QCGeom c = p->pc;
    c.ldc = ld ? ld : p->desc.M;
    QG_HIP(qg_launch_unpack_c(c, packed_dev, dst_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    return QG_OK;
}

static int execute_kernel(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, const qgemul_ep_args* epa, const HostC* hostc = nullptr);

int qgemul_execute(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB)
{
    if (!p || !packedC || !packedA || !packedB) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (p->has_ep) return QG_EINVAL;  // a plan with an epilogue runs through qgemul_execute_ep
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    QG_ON_DEVICE(p->ctx);
    return execute_kernel(p, packedC, packedA, packedB, nullptr);
}

// the kernels whose epilogue can store the reference layout: k_mfma_pp (QG_MFMA_PP) / k_mfma_ppl (QG_MFMA_PPL), real, 4- or 8-byte
// container equal to the host element, no raw-dot-product detour
bool stores_host_c(const qgemul_plan* p)
{
    if (p->has_ep || p->desc.is_complex || qg_wide_epilogue(p) || p->comp.on) return false;
    if (p->info.kernel != QG_KERNEL_MFMA_I8 && p->info.kernel != QG_KERNEL_MFMA_I8_LIMB) return false;
    if (p->variant != QG_MFMA_PP && p->variant != QG_MFMA_PPL && p->variant != QG_MFMA_K6) return false;
    if (p->variant == QG_MFMA_PPL && (p->pa.rows_p / p->cfg.TM) * (p->pb.rows_p / p->cfg.TN) < 256) return false;   // (falls back to the lock-step kernel)
    return (p->pc.cbytes == 4 || p->pc.cbytes == 8) && p->pc.cbytes == p->hc.size;
}

int qgemul_plan_stores_host_c(const qgemul_plan* p) { return p && stores_host_c(p) ? 1 : 0; }

int qgemul_execute_host_c(qgemul_plan* p, void* C_dev, int64_t ldc, const void* packedA, const void* packedB)
{
    if (!p || !C_dev || !packedA || !packedB || p->has_ep) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (ldc && ldc < p->desc.M) return QG_EINVAL;
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    QG_ON_DEVICE(p->ctx);
    if (stores_host_c(p)) {
        const HostC h{C_dev, ldc ? ldc : p->desc.M};
        return execute_kernel(p, C_dev, packedA, packedB, nullptr, &h);
    }
    if (!p->hostc_pc) QG_HIP(hipMalloc(&p->hostc_pc, (size_t)p->info.packed_bytes[2] ? (size_t)p->info.packed_bytes[2] : 16));
    const int st = execute_kernel(p, p->hostc_pc, packedA, packedB, nullptr);
    if (st != QG_OK) return st;
    QCGeom c = p->pc;
    c.ldc = ldc ? ldc : p->desc.M;
    QG_HIP(qg_launch_unpack_c(c, p->hostc_pc, C_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    return QG_OK;
}

static int ep_args_ok(const qgemul_plan* p, const qgemul_ep_args* args)
{
    if (!args && p->ept.n > 0) return QG_EINVAL;
    for (int k = 0; k < p->ept.n; ++k)
        if ((!p->ept.st[k].scalar || (p->ep_cplx && !p->ept_im.st[k].scalar)) && !args->e_packed[k]) return QG_EINVAL;
    return QG_OK;
}

// a chain as ONE linear pass over n elements: packed C (cbytes containers) -> packed D
static QEltwiseArgs chain_pass_args(const void* packedC, void* packedD, int64_t n, int cbytes, const QEpTable& t, const QEpArgs& a)
{
    QEltwiseArgs g;
    memset(&g, 0, sizeof g);
    g.C = (const char*)packedC;
    g.D = (char*)packedD;
    g.n = n;
    g.cbytes = cbytes;
    g.t = t;
    g.a = a;
    return g;
}

// ... with APPROX stages: the tables of `owner` (the plan that analysed the chain), the form choice of the caller's plan
static QApproxArgs approx_pass_args(const QEltwiseArgs& g, const qgemul_plan* owner, uint32_t flags)
{
    QApproxArgs x;
    memset(&x, 0, sizeof x);
    x.g = g;
    for (int k = 0; k < QG_MAX_EW; ++k) x.ax[k] = owner->ax_dev[k];
    x.force_general = (flags & QG_OPT_APPROX_GENERAL) ? 1 : 0;   // result-identical form choice (include/qgemul.h)
    return x;
}

// the plan's chain as ONE linear pass: packed C (the kernel's own layout and container, pc_c) -> packed D
static int run_chain_pass(qgemul_plan* p, const void* packedC, void* packedD, const QEpArgs& a, const qgemul_ep_args* args)
{
    hipStream_t st = p->ctx->stream;
    QEltwiseArgs g = chain_pass_args(packedC, packedD, p->pc_c.Mp * p->pc_c.Np, p->pc_c.cbytes, p->ept, a);
    if (p->has_ax) {
        QG_HIP(qg_launch_approx(approx_pass_args(g, p, p->flags), st));
        return QG_OK;
    }
    if (p->has_cmul) {
        // a CMUL stage needs both parts of an element in one thread: ONE pass whose lanes own both halves
        QCplxPassArgs x;
        memset(&x, 0, sizeof x);
        x.C = g.C;
        x.D = g.D;
        x.n = g.n;
        x.cbytes = g.cbytes;
        x.t[0] = p->ept;
        x.t[1] = p->ept_im;
        x.a = a;
        for (int k = 0; k < p->ept.n; ++k) x.scalar_im[k] = args->e_scalar_im[k];
        memcpy(x.e_cplx, p->e_cplx, sizeof x.e_cplx);
        x.cm = p->cm_dev;
        QG_HIP(qg_launch_eltwise_cplx(x, st));
        return QG_OK;
    }
    QG_HIP(qg_launch_eltwise(g, st));
    if (p->ep_cplx) {
        // the chain of the imaginary parts: the second half of packed C, of packed D and of every complex tensor operand
        g.C += g.n * g.cbytes;
        g.D += g.n * p->ept.dbytes;
        g.t = p->ept_im;
        for (int k = 0; k < p->ept_im.n; ++k) {
            if (g.a.e[k] && p->e_cplx[k]) g.a.e[k] += g.n * p->ept_im.st[k].ebytes;
            g.a.scalar[k] = args->e_scalar_im[k];
        }
        QG_HIP(qg_launch_eltwise(g, st));
    }
    return QG_OK;
}

static QEpArgs ep_device_args(const qgemul_plan* p, const qgemul_ep_args* args)
{
    QEpArgs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < p->ept.n; ++k) {
        a.e[k] = (const char*)args->e_packed[k];
        a.scalar[k] = args->e_scalar[k];
    }
    return a;
}

int qgemul_apply_epilogue(qgemul_plan* p, void* packedD, const void* packedC, const qgemul_ep_args* args)
{
    if (!p || !packedD || !packedC || !p->has_ep) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (int s = ep_args_ok(p, args)) return s;
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    QG_ON_DEVICE(p->ctx);
    return run_chain_pass(p, packedC, packedD, ep_device_args(p, args), args);
}

int qgemul_time_apply_epilogue(qgemul_plan* p, void* packedD, const void* packedC, const qgemul_ep_args* args, int warmup, int iters, float* avg_ms)
{
    if (!p || !avg_ms || iters < 1) return QG_EINVAL;
    return time_calls(p, warmup, iters, avg_ms, [&] { return qgemul_apply_epilogue(p, packedD, packedC, args); });
}

int qgemul_execute_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args)
{
    if (!p || !packedD || !packedA || !packedB) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (!p->has_ep) return args ? QG_EINVAL : qgemul_execute(p, packedD, packedA, packedB);
    if (int s = ep_args_ok(p, args)) return s;
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    QG_ON_DEVICE(p->ctx);
    const QEpArgs a = ep_device_args(p, args);
    hipStream_t st = p->ctx->stream;
    if (fuses_epilogue(p)) {
        // fused: the MFMA kernel's epilogue runs the chain on the value it has just converted into C's type
        QMfmaArgs m = mfma_args(p, packedA, packedB, packedD, p->pc_c.cbytes);
        m.has_ep = 1;
        m.ep = p->ept;
        m.epa = a;
        QG_HIP(qg_launch_mfma(p->LA, p->LB, m, st));
        return QG_OK;
    }
    // not fused: the kernel stores C into the plan's buffer, one linear pass turns it into D
    const int s = execute_kernel(p, p->cwork, packedA, packedB, nullptr);
    if (s != QG_OK) return s;
    return run_chain_pass(p, p->cwork, packedD, a, args);
}

int qgemul_plan_fuses_epilogue(const qgemul_plan* p)
{
    if (p && p->grp) return p->grp->has_ep && p->grp->fused && p->grp->n_in ? 1 : 0;   // (the members in the launch)
    if (p && p->batch) return p->has_ep && (p->bd ? p->bd_fused : fuses_epilogue(p->member)) ? 1 : 0;
    return p && p->has_ep && fuses_epilogue(p) ? 1 : 0;
}

int qgemul_plan_packed_layout(const qgemul_plan* p, int operand, int64_t out[4])
{
    if (!p || !out || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    if (p->grp) return QG_EINVAL;   // a grouped plan answers qgemul_plan_grouped_member
    const QPackedGeom& g = operand == QG_OPERAND_A ? p->pa : p->pb;
    out[0] = p->comp.on ? 0 : g.trailer;
    out[1] = g.offs ? g.rowsum_off : 0;
    out[2] = g.rows_p;
    out[3] = g.offs ? -g.bias : 0;
    return QG_OK;
}

// the stage entry that reads stage k's tensor operand (nullptr: the stage has no tensor operand)
static const QEpStage* stage_tensor(const qgemul_plan* p, int k)
{
    if (!p->ept.st[k].scalar) return &p->ept.st[k];
    if (p->ep_cplx && !p->ept_im.st[k].scalar) return &p->ept_im.st[k];
    return nullptr;
}

int64_t qgemul_packed_c_bytes(const qgemul_plan* p)
{
    return p && p->has_ep && p->batch < 1 ? (int64_t)p->pc_c.parts * p->pc_c.Mp * p->pc_c.Np * p->pc_c.cbytes : 0;
}

// a tensor of the GEMM result's own element type -> the packed C the chain's pass reads (qgemul_apply_epilogue)
int qgemul_pack_c(qgemul_plan* p, const void* src_dev, int64_t ld, void* packed_dev)
{
    if (!p || !src_dev || !packed_dev || !p->has_ep) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    if (ld && ld < p->desc.M) return QG_EINVAL;
    QG_ON_DEVICE(p->ctx);
    const QHostElem h = qg_host_elem(p->desc.c, p->desc.is_complex);
    for (int part = 0; part < p->pc_c.parts; ++part)
        QG_HIP(qg_launch_pack_e(p->pc_c, part, src_dev, ld ? ld : p->desc.M, h.size, h.off[part], h.sb[part], packed_dev, p->pc_c.cbytes, p->ctx->stream));
    return QG_OK;
}

int64_t qgemul_packed_e_bytes(const qgemul_plan* p, int stage)
{
    if (!p || !p->has_ep || stage < 0 || stage >= p->ept.n) return 0;
    if (p->grp) return p->grp->ebytes[stage];   // (the whole group's)
    if (p->batch) return p->e_shared[stage] ? p->estride[stage] : p->batch * p->estride[stage];   // (one member's / the stack's)
    const QEpStage* t = stage_tensor(p, stage);
    if (!t) return 0;
    return (p->ep_cplx && p->e_cplx[stage] ? 2 : 1) * p->pc.Mp * p->pc.Np * (int64_t)t->ebytes;
}

int qgemul_pack_e(qgemul_plan* p, int stage, const void* src_dev, int64_t ld, void* packed_dev)
{
    if (!p || !src_dev || !packed_dev || !p->has_ep || stage < 0 || stage >= p->ept.n) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    const QEpStage* t = stage_tensor(p, stage);
    if (!t) return QG_EINVAL;
    if (ld && ld < p->desc.M) return QG_EINVAL;
    QG_ON_DEVICE(p->ctx);
    const bool cplx = p->ep_cplx && p->e_cplx[stage];
    // host element of the operand tensor: int32 / int64 raw values, {re, im} structs for a complex operand (QuBLAS.h:2512-2513)
    const qfmt f[2] = {t == &p->ept.st[stage] ? p->ep.stage[stage].e : p->ep_im.stage[stage].e, p->ep_im.stage[stage].e};
    const QHostElem h = qg_host_elem(f, cplx ? 1 : 0);
    for (int part = 0; part < (cplx ? 2 : 1); ++part)
        QG_HIP(qg_launch_pack_e(p->pc, part, src_dev, ld ? ld : p->desc.M, h.size, h.off[part], h.sb[part], packed_dev, t->ebytes, p->ctx->stream));
    return QG_OK;
}

// composite linear plan: per k-chunk, one MFMA launch per (A group, B group) storing raw dot products into its slab, then the
// exact combine pass (running sums between chunks; one round + overflow into C after the last)
static int execute_composite(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, const QCGeom& pcg)
{
    const QComposite& q = p->comp;
    hipStream_t st = p->ctx->stream;
    const int64_t n = p->pa.rows_p * p->pb.rows_p;
    for (int c = 0; c < q.nc; ++c) {
        QLinCombine cb;
        memset(&cb, 0, sizeof cb);
        for (int i = 0; i < q.ga; ++i)
            for (int j = 0; j < q.gb; ++j) {
                int64_t offA = 0, offB = 0;
                const QPackedGeom sa = qg_comp_sub_geom(q, p->pa, 0, p->desc.K, c, i, &offA);
                const QPackedGeom sb = qg_comp_sub_geom(q, p->pb, 1, p->desc.K, c, j, &offB);
                char* slab = (char*)p->comp_slabs + (size_t)(i * q.gb + j) * (size_t)n * (size_t)q.slab_bytes;
                QMfmaArgs a = mfma_args(sa, sb, q.var[i][j], (const char*)packedA + offA, (const char*)packedB + offB, slab, q.slab_bytes);
                a.to_c.identity = 1;   // raw dot products
                QG_HIP(qg_launch_mfma(sa.limbs, sb.limbs, a, st));
                cb.slab[cb.n_slabs] = slab;
                cb.sh[cb.n_slabs] = 8 * (sa.limb0 + sb.limb0);
                ++cb.n_slabs;
            }
        cb.slab_bytes = q.slab_bytes;
        cb.n = n;
        cb.acc_in = c > 0 ? p->comp_acc : nullptr;
        cb.acc_out = c + 1 < q.nc ? p->comp_acc : nullptr;
        cb.out = packedC;
        cb.cbytes = pcg.cbytes;
        cb.wide = q.wide;
        cb.to_c = p->an.lin.to_c[0];
        if (p->pa.offs) {   // centred operands: the last chunk's pass takes the centres back out
            cb.rsA = (const int64_t*)((const char*)packedA + p->pa.rowsum_off);
            cb.rsB = (const int64_t*)((const char*)packedB + p->pb.rowsum_off);
            cb.biasA = p->pa.bias;
            cb.biasB = p->pb.bias;
            cb.corr = p->desc.K;
            cb.tm = pcg.tm;
            cb.tn = pcg.tn;
            cb.tiles_n = pcg.tn ? pcg.Np / pcg.tn : 1;
        }
        QG_HIP(qg_launch_lin_combine(cb, st));
    }
    return QG_OK;
}

static int execute_kernel(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, const qgemul_ep_args*, const HostC* hostc)
{
    hipStream_t st = p->ctx->stream;
    const QCGeom& pcg = p->has_ep ? p->pc_c : p->pc;
    if (p->comp.on) return execute_composite(p, packedC, packedA, packedB, pcg);
    switch (p->info.kernel) {
    case QG_KERNEL_MFMA_I8:
    case QG_KERNEL_MFMA_I8_LIMB: {
        if (p->variant == QG_MFMA_RING) {
            QRingArgs r;
            memset(&r, 0, sizeof r);
            r.A = (const int8_t*)packedA;
            r.B = (const int8_t*)packedB;
            r.C = packedC;
            r.Mp = p->pa.rows_p;
            r.Np = p->pb.rows_p;
            r.Kp = p->pa.K_p;
            r.cbytes = pcg.cbytes;
            r.n = p->an.ring_n;
            r.s = p->an.ring_s;
            r.to_c = p->an.tree.c_cvt[0];
            QG_HIP(qg_launch_mfma_ring(p->LA, p->LB, qg_ring_digits(p->an.ring_n), r, st));
            return QG_OK;
        }
        QMfmaArgs a = mfma_args(p, packedA, packedB, packedC, pcg.cbytes);
#ifdef QG_DIAG
        a.dbg = g_diag_stamps;
#endif
        if (p->pa.digit6) {
            a.kara = 1;   // (row sums, biases and corr: centre_args)
            a.Mc = pcg.Mp;
        }
        if (qg_wide_epilogue(p)) {
            a.C = p->wide_ws;
            a.cbytes = 4;
            memset(&a.to_c, 0, sizeof a.to_c);
            a.to_c.identity = 1;                    // raw int32 dot products ...
            QG_HIP(qg_launch_mfma(p->LA, p->LB, a, st));
            QEltwiseArgs f;
            memset(&f, 0, sizeof f);
            f.C = (const char*)p->wide_ws;
            f.D = (char*)packedC;
            f.n = pcg.Mp * pcg.Np;
            f.cbytes = 4;
            f.t.dbytes = pcg.cbytes;
            f.t.to_d = p->an.lin.to_c[0];           // ... shifted, overflow-handled and stored in 64-bit arithmetic
            QG_HIP(qg_launch_eltwise(f, st));
            return QG_OK;
        }
        if (hostc) {   // (only reached when stores_host_c(p): see qgemul_execute_host_c)
            a.C = hostc->C;
            a.c_host = 1;
            a.c_ld = hostc->ld;
            a.c_M = p->desc.M;
            a.c_N = p->desc.N;
            a.c_vec = (((uintptr_t)hostc->C & 15) == 0 && (hostc->ld * pcg.cbytes) % 16 == 0) ? 1 : 0;
        }
        QG_HIP(qg_launch_mfma(p->LA, p->LB, a, st));
        return QG_OK;
    }
    case QG_KERNEL_MFMA_CPLX: {
        QMfmaArgs a = mfma_args(p->pa, p->pb, p->variant, packedA, packedB, p->workspace, 8);
        a.Mp = 2 * p->pa.rows_p;   // the parts stacked along the rows: one real GEMM of twice the extents
        a.Np = 2 * p->pb.rows_p;
        a.to_c.identity = 1;  // raw 64-bit dot products
        QG_HIP(qg_launch_mfma(p->LA, p->LB, a, st));
        QCplxCombine g;
        g.D = p->workspace;
        g.C = (char*)packedC;
        g.M = p->desc.M;
        g.N = p->desc.N;
        g.Mh = p->pa.rows_p;
        g.Nh = p->pb.rows_p;
        g.Np = 2 * p->pb.rows_p;
        g.tm = p->cfg.TM;
        g.tn = p->cfg.TN;
        g.cbytes = pcg.cbytes;
        for (int i = 0; i < 4; ++i) g.sh[i] = p->an.lin.sh[i];
        g.to_c[0] = p->an.lin.to_c[0];
        g.to_c[1] = p->an.lin.to_c[1];
        QG_HIP(qg_launch_cplx_combine(g, st));
        return QG_OK;
    }
    case QG_KERNEL_MFMA_RC: {
        const bool ca = p->desc.cmul == QG_CMUL_REAL_B;   // A is the complex operand
        QMfmaArgs a = mfma_args(p->pa, p->pb, p->variant, packedA, packedB, p->workspace, 8);
        a.Mp = (ca ? 2 : 1) * p->pa.rows_p;   // the complex operand's parts stacked along its rows: one real GEMM
        a.Np = (ca ? 1 : 2) * p->pb.rows_p;
        a.to_c.identity = 1;  // raw 64-bit dot products
        QG_HIP(qg_launch_mfma(p->LA, p->LB, a, st));
        QRcConvert g;
        g.D = p->workspace;
        g.C = (char*)packedC;
        g.M = p->desc.M;
        g.N = p->desc.N;
        g.Np = a.Np;
        g.im_r = ca ? p->pa.rows_p : 0;
        g.im_c = ca ? 0 : p->pb.rows_p;
        g.tm = p->cfg.TM;
        g.tn = p->cfg.TN;
        g.cbytes = pcg.cbytes;
        g.to_c[0] = p->an.lin.to_c[0];
        g.to_c[1] = p->an.lin.to_c[1];
        QG_HIP(qg_launch_rc_convert(g, st));
        return QG_OK;
    }
    case QG_KERNEL_TREE_I32:
        QG_HIP(qg_launch_tree_fast(p->dev_table, p->an.tree.n_levels_k, p->an.split_s, p->an.mul24_ok, p->tc.tree, packedA, packedB, packedC,
                                   p->desc.M, p->desc.N, p->pa.K_p, pcg.cbytes, st));
        return QG_OK;
    case QG_KERNEL_GEMV_I64:
        QG_HIP(qg_launch_gemv(p->dev_table, p->an.tree.n_levels_k, p->an.gemv_b_bit, QGF_RUNTIME, packedA, packedB, packedC, p->desc.M, p->pa.K_p,
                              pcg.cbytes, st, 1));
        return QG_OK;
    case QG_KERNEL_GEMV_I32:
        QG_HIP(qg_launch_gemv(p->dev_table, p->an.tree.n_levels_k, p->an.gemv_b_bit, p->tc.gemv, packedA, packedB, packedC, p->desc.M, p->pa.K_p,
                              pcg.cbytes, st));
        return QG_OK;
    case QG_KERNEL_TREE_CPLX_I32:
        QG_HIP(qg_launch_tree_cplx_fast(p->dev_table, p->an.tree.n_levels_k, p->tc.cplx, p->desc.cmul == QG_CMUL_TF ? 1 : 0, packedA, packedB, packedC,
                                        p->desc.M, p->desc.N, p->pa.K_p, pcg.cbytes, st));
        return QG_OK;
    case QG_KERNEL_TREE_RC_I32:
        QG_HIP(qg_launch_tree_rc(p->dev_table, p->an.tree.n_levels_k, p->tc.cplx, p->desc.cmul == QG_CMUL_REAL_B ? 1 : 0, packedA, packedB, packedC, p->desc.M,
                                 p->desc.N, p->pa.K_p, pcg.cbytes, st));
        return QG_OK;
    case QG_KERNEL_TREE_I64:
        if (p->an.tree64_ok && !(p->flags & QG_OPT_GENERIC_TREE)) {
            QG_HIP(qg_launch_tree64(p->dev_table, p->an.tree.n_levels_k, packedA, packedB, packedC, p->desc.M, p->desc.N, p->pa.K_p,
                                    p->pa.cbytes, p->pb.cbytes, pcg.cbytes, st));
            return QG_OK;
        }
        [[fallthrough]];
    case QG_KERNEL_TREE_CPLX:
        QG_HIP(qg_launch_tree_generic(p->dev_table, p->desc.is_complex ? 2 : 1, packedA, packedB, packedC, p->desc.M, p->desc.N,
                                      p->desc.K, p->pa, p->pb, pcg, st));
        return QG_OK;
    case QG_KERNEL_TREE_I128:
        QG_HIP(qg_launch_tree_generic(p->dev_table, p->desc.is_complex ? 2 : 1, packedA, packedB, packedC, p->desc.M, p->desc.N,
                                      p->desc.K, p->pa, p->pb, pcg, st, 1));
        return QG_OK;
    default:
        return QG_EUNSUPPORTED;
    }
}

static int result_width(const qgemul_plan* p, int part = 0)
{
    const qfmt f = p->has_ep ? (part ? p->ep_im.d : p->ep.d) : p->desc.c[part];
    return (int)f.I + (int)f.F + (f.S ? 1 : 0);
}

int64_t qgemul_bitstream_bytes(const qgemul_plan* p, int format)
{
    if (!p || p->batch) return 0;
    const int64_t n = p->desc.M * p->desc.N;
    // complex: "(re-bits, im-bits)" per element as characters; packed: the binary characters only
    const int64_t bits = p->desc.is_complex ? n * (result_width(p, 0) + result_width(p, 1) + (format == QG_BITS_PACKED ? 0 : 4)) : n * (int64_t)result_width(p);
    // the packed form is written with 32-bit atomics: sized to whole words
    return format == QG_BITS_PACKED ? ((bits + 7) / 8 + 3) / 4 * 4 : bits;
}

int qgemul_export_bitstream(qgemul_plan* p, const void* packedC, int tensor_chunk, int elem_chunk, int format, void* out_dev)
{
    if (!p || !packedC || !out_dev || (format != QG_BITS_ASCII && format != QG_BITS_PACKED)) return QG_EINVAL;
    if (p->batch) return QG_EINVAL;   // a batched plan runs through the _batched entry points
    const int w = p->desc.is_complex ? result_width(p, 0) + result_width(p, 1) + 4 : result_width(p);
    const int64_t n = p->desc.M * p->desc.N;
    if (w <= 0 || tensor_chunk < 0 || elem_chunk < 0) return QG_EINVAL;
    if (!p->desc.is_complex && (w > 64 || p->pc.cbytes > 8)) return QG_EUNSUPPORTED;   // (multi-word elements: not exported)
    if (elem_chunk > 0 && w % elem_chunk) return QG_EINVAL;      // the reference throws (QuBLAS.h:4599-4602)
    if (tensor_chunk > 0 && n % tensor_chunk) return QG_EINVAL;  // the reference's loop does not terminate (:4745)
    QG_ON_DEVICE(p->ctx);
    if (p->desc.is_complex) {
        const int wr = result_width(p, 0), wi = result_width(p, 1);
        if (wr < 0 || wi < 0 || wr > 64 || wi > 64) return QG_EINVAL;   // (a part without bits prints as the empty string)
        QBitsCplxArgs a;
        memset(&a, 0, sizeof a);
        a.c = p->pc;
        a.packed = (const char*)packedC;
        a.out = (char*)out_dev;
        a.width = w;
        a.nbits = wr + wi;
        a.tensor_chunk = tensor_chunk;
        a.packed_bits = format == QG_BITS_PACKED;
        // the element string "(" re ", " im ")" (QuBLAS.h:2553-2556), MSB first per part, then its chunks reversed (:4593-4611)
        uint8_t str[136];
        int k = 0;
        str[k++] = QG_BITS_LIT_OPEN;
        for (int j = 0; j < wr; ++j) str[k++] = (uint8_t)(wr - 1 - j);
        str[k++] = QG_BITS_LIT_COMMA;
        str[k++] = QG_BITS_LIT_SPACE;
        for (int j = 0; j < wi; ++j) str[k++] = (uint8_t)(64 + wi - 1 - j);
        str[k++] = QG_BITS_LIT_CLOSE;
        if (elem_chunk > 0) {
            const int nch = w / elem_chunk;
            for (int q = 0; q < nch; ++q)
                for (int r = 0; r < elem_chunk; ++r) a.tab[q * elem_chunk + r] = str[(nch - 1 - q) * elem_chunk + r];
        } else {
            memcpy(a.tab, str, (size_t)w);
        }
        QG_HIP(qg_launch_bitstream_cplx(a, p->ctx->stream));
        return QG_OK;
    }
    QBitsArgs a;
    memset(&a, 0, sizeof a);
    a.c = p->pc;
    a.packed = (const char*)packedC;
    a.out = (char*)out_dev;
    a.width = w;
    a.tensor_chunk = tensor_chunk;
    a.elem_chunk = elem_chunk;
    a.packed_bits = format == QG_BITS_PACKED;
    QG_HIP(qg_launch_bitstream(a, p->ctx->stream));
    return QG_OK;
}

// the plan a timing entry point is for (a batched plan's chain is told by the plan; a grouped plan's by the entry point)
enum TimedPlan { TIMED_PLAIN, TIMED_BATCHED, TIMED_GROUPED, TIMED_GROUPED_EP };

static int time_execute(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, const qgemul_ep_args* args,
                        int warmup, int iters, float* avg_ms, TimedPlan kind = TIMED_PLAIN)
{
    const bool batched = kind == TIMED_BATCHED, grouped = kind == TIMED_GROUPED || kind == TIMED_GROUPED_EP;
    if (!p || !avg_ms || iters < 1 || (grouped ? !p->grp : (p->batch != 0) != batched)) return QG_EINVAL;
    return time_calls(p, warmup, iters, avg_ms, [&] {
        if (kind == TIMED_GROUPED_EP) return qgemul_execute_grouped_ep(p, packedC, packedA, packedB, args);
        if (kind == TIMED_GROUPED) return qgemul_execute_grouped(p, packedC, packedA, packedB);
        if (batched) return p->has_ep ? qgemul_execute_batched_ep(p, packedC, packedA, packedB, args) : qgemul_execute_batched(p, packedC, packedA, packedB);
        return p->has_ep ? qgemul_execute_ep(p, packedC, packedA, packedB, args) : qgemul_execute(p, packedC, packedA, packedB);
    });
}

int qgemul_time_execute(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int warmup, int iters,
                        float* avg_ms)
{
    return time_execute(p, packedC, packedA, packedB, nullptr, warmup, iters, avg_ms);
}

int qgemul_time_execute_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args,
                           int warmup, int iters, float* avg_ms)
{
    return time_execute(p, packedD, packedA, packedB, args, warmup, iters, avg_ms);
}


// ---- batched Qgemul: `batch` GEMMs of one descriptor at constant strides (include/qgemul.h) ----
// what qg_batched_geometry fills (zeroed; on the heap: a QPlanGeom holds the whole analysis)
struct BatchedGeoms { QPlanGeom m, s; QBatchGeom b; };

int classify_batched_view(const qgemul_desc* d, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_info* out, int* launches)
{
    if (!d) return QG_EINVAL;
    BatchedGeoms* g = new (std::nothrow) BatchedGeoms();
    if (!g) return QG_EINVAL;
    const int st = qg_batched_geometry(d, batch, opt_flags, ev, bep, &g->m, &g->s, &g->b);
    if (out && batch >= 1) *out = g->s.info;
    if (launches && st == QG_OK) *launches = qg_batched_launches(&g->s, &g->b, ev != nullptr);
    delete g;
    return st;
}

int qgemul_classify_batched(const qgemul_desc* d, int64_t batch, uint32_t opt_flags, qgemul_info* out)
{
    if (!d || !out) return QG_EINVAL;
    return classify_batched_view(d, batch, nullptr, nullptr, opt_flags, out, nullptr);
}

int qgemul_classify_batched_launches(const qgemul_desc* d, int64_t batch, uint32_t opt_flags)
{
    int n = 0;
    const int st = classify_batched_view(d, batch, nullptr, nullptr, opt_flags, nullptr, &n);
    return st == QG_OK ? n : st;
}

// the member owns every device resource (with a chain: its device tables as well) except the block-diagonal pass form's packed C
int plan_create_batched_view(qgemul_ctx* c, const qgemul_desc* d, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_plan** out)
{
    if (!c || !d || !out) return QG_EINVAL;
    BatchedGeoms* g = new (std::nothrow) BatchedGeoms();
    qgemul_plan* b = new (std::nothrow) qgemul_plan();
    int st = g && b ? qg_batched_geometry(d, batch, opt_flags, ev, bep, &g->m, &g->s, &g->b) : QG_EINVAL;
    if (st == QG_OK) {
        static_cast<QPlanGeom&>(*b) = g->s;
        static_cast<QBatchGeom&>(*b) = g->b;
        b->desc = *d;
        b->flags = opt_flags;
        if (ev) {   // the chain is the member's
            b->has_ep = 1;
            b->ep = *ev->re;
            for (int k = 0; ev->ax && k < QG_MAX_EW; ++k) b->has_ax |= ev->ax[k] != nullptr;
        }
        st = plan_create_view(c, d, ev, opt_flags, &b->member, batch);
    }
    delete g;
    if (st != QG_OK) { delete b; return st; }
    b->ctx = c;
    if (b->has_ep && b->bd && !b->bd_fused) {   // the pass form: the stack's packed C between the two launches
        DeviceScope scope(c->device);
        const size_t cb = (size_t)batch * (size_t)(b->pc_c.Mp * b->pc_c.Np) * (size_t)b->pc_c.cbytes;
        if (scope.err != hipSuccess || hipMalloc(&b->cwork, cb ? cb : 16) != hipSuccess) {
            qgemul_plan_destroy(b);
            return QG_EHIP;
        }
    }
    if (b->bd_stack) {   // the stacked form: the raw dot products between its two launches
        DeviceScope scope(c->device);
        if (scope.err != hipSuccess || hipMalloc((void**)&b->stack_work, (size_t)(b->stack_ws ? b->stack_ws : 16)) != hipSuccess) {
            qgemul_plan_destroy(b);
            return QG_EHIP;
        }
    }
    *out = b;
    return QG_OK;
}

int qgemul_plan_create_batched(qgemul_ctx* c, const qgemul_desc* d, int64_t batch, uint32_t opt_flags, qgemul_plan** out)
{
    return plan_create_batched_view(c, d, batch, nullptr, nullptr, opt_flags, out);
}

int qgemul_plan_batched_launches(const qgemul_plan* p)
{
    if (!p || p->batch < 1) return QG_EINVAL;
    return qg_batched_launches(p, p, p->has_ep != 0);
}

int qgemul_pack_batched(qgemul_plan* p, int operand, const void* src_dev, int64_t ld, int64_t member_stride, void* packed_dev)
{
    if (!p || p->batch < 1 || !src_dev || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    const int64_t ext = qg_member_extent(p->desc, operand, ld);
    if (ext < 1 || member_stride < ext) return QG_EINVAL;
    qgemul_plan* m = p->member;
    const int64_t eb = operand == QG_OPERAND_A ? p->ha.size : p->hb.size;
    if (!p->bd && !p->bd_stack) {
        for (int64_t b = 0; b < p->batch; ++b)
            if (const int st = qgemul_pack(m, operand, (const char*)src_dev + b * member_stride * eb, ld, (char*)packed_dev + b * p->mstride[operand]); st != QG_OK) return st;
        return QG_OK;
    }
    QG_ON_DEVICE(p->ctx);
    const QOperandGeom g = operand_geom(m, operand, ld);
    const int check = (p->flags & QG_OPT_CHECK_RANGE) ? 1 : 0;
    if (const int st = range_check_begin(p, check); st != QG_OK) return st;
    QG_HIP(qg_launch_pack_stack(g, operand == QG_OPERAND_A ? m->pa : m->pb, operand == QG_OPERAND_A ? p->pa : p->pb, p->batch, src_dev, member_stride * eb,
                                packed_dev, check, p->ctx->flag_dev, p->ctx->stream, (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
    return range_check_end(p, check);
}

int qgemul_unpack_c_batched(qgemul_plan* p, const void* packed_dev, void* dst_dev, int64_t ld, int64_t member_stride)
{
    if (!p || p->batch < 1 || !packed_dev || !dst_dev) return QG_EINVAL;
    const int64_t ext = qg_member_extent(p->desc, QG_OPERAND_C, ld);
    if (ext < 1 || member_stride < ext) return QG_EINVAL;
    for (int64_t b = 0; b < p->batch; ++b)   // (a layout step: one launch per member, the members' packed Cs back to back)
        if (const int st = qgemul_unpack_c(p->member, (const char*)packed_dev + b * p->mstride[2], (char*)dst_dev + b * member_stride * p->hc.size, ld); st != QG_OK) return st;
    return QG_OK;
}

// the block-diagonal launch of a batched plan: the stack is a packed A and a packed B, with its own plane masks and row sums, and the
// member's conversion into C
static QMfmaArgs bd_mfma_args(const qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int cbytes)
{
    const qgemul_plan* m = p->member;
    QMfmaArgs a = mfma_args(p->pa, p->pb, p->variant, packedA, packedB, packedC, cbytes);
    a.to_c = m->an.lin.to_c[0];
    centre_args(a, p->pa, p->pb, packedA, packedB, p->desc.K);
    a.bd_tm = (int32_t)(m->pa.rows_p / p->cfg.TM);
    a.bd_tn = (int32_t)(m->pb.rows_p / p->cfg.TN);
    return a;
}

// the stacked form (QG_OPT_BATCHED_STACKED): the members' stacked parts as ONE block-diagonal GEMM of raw 64-bit dot products into the
// plan's workspace — member blocks of bd_tm x bd_tn tiles —, then ONE combine pass into the members' packed Cs (qg_combine_bd.hip)
// which: -1 both launches; 0 / 1: that launch alone (qgemul_time_execute_batched_launch: the measurement of the two shares)
static int execute_stacked(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int which = -1)
{
    const qgemul_plan* m = p->member;
    QG_ON_DEVICE(p->ctx);
    QMfmaArgs a = mfma_args(p->pa, p->pb, p->variant, packedA, packedB, p->stack_work, 8);
    a.to_c.identity = 1;
    a.bd_tm = p->bd_tm;
    a.bd_tn = p->bd_tn;
    if (which != 1) QG_HIP(qg_launch_mfma_bd(p->LA, p->LB, a, p->batch, p->ctx->stream));
    if (which == 0) return QG_OK;
    QStackCombine g;
    memset(&g, 0, sizeof g);
    g.W = p->stack_work;
    g.C = (char*)packedC;
    g.M = p->desc.M;
    g.N = p->desc.N;
    g.cstride = p->mstride[2];
    g.tm = (int32_t)(m->pa.rows_p / p->cfg.TM);
    g.tn = (int32_t)(m->pb.rows_p / p->cfg.TN);
    g.bd_tm = p->bd_tm;
    g.bd_tn = p->bd_tn;
    g.im_r = p->bd_stack == QG_STACK_REAL_B ? g.tm : 0;
    g.im_c = p->bd_stack == QG_STACK_REAL_A ? g.tn : 0;
    g.mode = p->bd_stack;
    g.cbytes = p->pc.cbytes;
    for (int i = 0; i < 4; ++i) g.sh[i] = m->an.lin.sh[i];
    g.to_c[0] = m->an.lin.to_c[0];
    g.to_c[1] = m->an.lin.to_c[1];
    QG_HIP(qg_launch_stack_combine_bd(g, p->batch, p->ctx->stream));
    return QG_OK;
}

int qgemul_execute_batched(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB)
{
    if (!p || p->batch < 1 || !packedC || !packedA || !packedB) return QG_EINVAL;
    if (p->has_ep) return QG_EINVAL;  // a batched plan with a chain runs through qgemul_execute_batched_ep
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    qgemul_plan* m = p->member;
    if (p->bd_stack) return execute_stacked(p, packedC, packedA, packedB);
    if (p->bd_tree) {   // QG_OPT_BATCHED_TREE: ONE launch of the member's tree kernel's batched twin, the members at their packed strides
        QG_ON_DEVICE(p->ctx);
        if (m->info.kernel == QG_KERNEL_TREE_I32)
            QG_HIP(qg_launch_tree_fast_bd(m->dev_table, m->an.tree.n_levels_k, m->an.split_s, m->an.mul24_ok, m->tc.tree, packedA, packedB, packedC, m->desc.M,
                                          m->desc.N, m->pa.K_p, m->pc.cbytes, p->batch, p->mstride, p->ctx->stream));
        else
            QG_HIP(qg_launch_tree_cplx_fast_bd(m->dev_table, m->an.tree.n_levels_k, m->tc.cplx, m->desc.cmul == QG_CMUL_TF ? 1 : 0, packedA, packedB, packedC,
                                               m->desc.M, m->desc.N, m->pa.K_p, m->pc.cbytes, p->batch, p->mstride, p->ctx->stream));
        return QG_OK;
    }
    if (!p->bd) {
        for (int64_t b = 0; b < p->batch; ++b)
            if (const int st = qgemul_execute(m, (char*)packedC + b * p->mstride[2], (const char*)packedA + b * p->mstride[0], (const char*)packedB + b * p->mstride[1]); st != QG_OK)
                return st;
        return QG_OK;
    }
    QG_ON_DEVICE(p->ctx);
    const QMfmaArgs a = bd_mfma_args(p, packedC, packedA, packedB, p->pc.cbytes);
    QG_HIP(qg_launch_mfma_bd(p->LA, p->LB, a, p->batch, p->ctx->stream));
    return QG_OK;
}

int qgemul_time_execute_batched(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int warmup, int iters, float* avg_ms)
{
    if (p && p->has_ep) return QG_EINVAL;
    return time_execute(p, packedC, packedA, packedB, nullptr, warmup, iters, avg_ms, TIMED_BATCHED);
}

int qgemul_time_execute_batched_launch(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int launch, int warmup, int iters, float* avg_ms)
{
    if (!p || p->batch < 1 || !p->bd_stack || !packedC || !packedA || !packedB || !avg_ms || iters < 1 || (launch != 0 && launch != 1)) return QG_EINVAL;
    if (p->desc.M == 0 || p->desc.N == 0) { *avg_ms = 0; return QG_OK; }
    return time_calls(p, warmup, iters, avg_ms, [&] { return execute_stacked(p, packedC, packedA, packedB, launch); });
}

// ---- element-wise chains on batched plans (include/qgemul.h): member b is Qgemul<...>(C_b, A_b, B_b) followed by the chain ----
// (ax == nullptr: a chain without APPROX stages)
static const qgemul_approx* const g_no_ax[QG_MAX_EW] = {};

int qgemul_classify_batched_epx(const qgemul_desc* d, int64_t batch, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_info* out)
{
    if (!out || !ep) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax ? ax : g_no_ax};
    return classify_batched_view(d, batch, &v, bep, opt_flags, out, nullptr);
}

int qgemul_classify_batched_epx_launches(const qgemul_desc* d, int64_t batch, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                         const qgemul_batched_ep* bep, uint32_t opt_flags)
{
    if (!ep) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax ? ax : g_no_ax};
    int n = 0;
    const int st = classify_batched_view(d, batch, &v, bep, opt_flags, nullptr, &n);
    return st == QG_OK ? n : st;
}

int qgemul_plan_create_batched_epx(qgemul_ctx* c, const qgemul_desc* d, int64_t batch, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                   const qgemul_batched_ep* bep, uint32_t opt_flags, qgemul_plan** out)
{
    if (!c || !d || !ep || !out) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax ? ax : g_no_ax};
    return plan_create_batched_view(c, d, batch, &v, bep, opt_flags, out);
}

int qgemul_pack_e_batched(qgemul_plan* p, int stage, const void* src_dev, int64_t ld, int64_t member_stride, void* packed_dev)
{
    if (!p || p->batch < 1 || !p->has_ep || !src_dev || !packed_dev || stage < 0 || stage >= p->ept.n) return QG_EINVAL;
    if (!p->estride[stage]) return QG_EINVAL;   // a scalar or APPROX stage has no tensor operand
    const int64_t ext = qg_member_extent(p->desc, QG_OPERAND_C, ld);
    if (ext < 1) return QG_EINVAL;
    if (p->e_shared[stage] ? member_stride != 0 : member_stride < ext) return QG_EINVAL;
    const qfmt f[2] = {p->ep.stage[stage].e, p->ep.stage[stage].e};
    const int64_t eb = qg_host_elem(f, 0).size;
    const int64_t n = p->e_shared[stage] ? 1 : p->batch;
    for (int64_t b = 0; b < n; ++b)   // (a layout step like qgemul_unpack_c_batched: one launch per member)
        if (const int st = qgemul_pack_e(p->member, stage, (const char*)src_dev + b * member_stride * eb, ld, (char*)packed_dev + b * p->estride[stage]); st != QG_OK) return st;
    return QG_OK;
}

int qgemul_execute_batched_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args)
{
    if (!p || p->batch < 1 || !p->has_ep || !packedD || !packedA || !packedB) return QG_EINVAL;
    if (int s = ep_args_ok(p, args)) return s;
    if (p->desc.M == 0 || p->desc.N == 0) return QG_OK;
    qgemul_plan* m = p->member;
    if (!p->bd) {
        for (int64_t b = 0; b < p->batch; ++b) {
            qgemul_ep_args ma;
            memset(&ma, 0, sizeof ma);
            for (int k = 0; k < p->ept.n; ++k) {
                ma.e_scalar[k] = args->e_scalar[k];
                if (p->estride[k]) ma.e_packed[k] = (const char*)args->e_packed[k] + (p->e_shared[k] ? 0 : b * p->estride[k]);
            }
            if (const int st = qgemul_execute_ep(m, (char*)packedD + b * p->mstride[2], (const char*)packedA + b * p->mstride[0], (const char*)packedB + b * p->mstride[1], &ma); st != QG_OK)
                return st;
        }
        return QG_OK;
    }
    QG_ON_DEVICE(p->ctx);
    hipStream_t st = p->ctx->stream;
    QBdEp be;
    memset(&be, 0, sizeof be);
    be.msize = p->pc_c.Mp * p->pc_c.Np;
    for (int k = 0; k < p->ept.n; ++k)
        if (p->estride[k] && p->e_shared[k]) be.shared |= 1u << k;
    const QEpArgs ea = ep_device_args(p, args);
    if (p->bd_fused) {
        // ONE launch: the block-diagonal kernel's epilogue runs the chain on the value it has just converted into C's type
        QMfmaEpBdArgs a;
        memset(&a, 0, sizeof a);
        (QMfmaArgs&)a = bd_mfma_args(p, packedD, packedA, packedB, p->pc_c.cbytes);
        a.has_ep = 1;
        a.ep = p->ept;
        a.epa = ea;
        a.bd = be;
        QG_HIP(qg_launch_mfma_ep_bd(p->LA, p->LB, a, p->batch, st));
        return QG_OK;
    }
    // TWO launches: the block-diagonal kernel as it is into the plan's packed C of the whole stack, then ONE pass over the stack
    const QMfmaArgs a = bd_mfma_args(p, p->cwork, packedA, packedB, p->pc_c.cbytes);
    QG_HIP(qg_launch_mfma_bd(p->LA, p->LB, a, p->batch, st));
    const QEltwiseArgs g = chain_pass_args(p->cwork, packedD, p->batch * be.msize, p->pc_c.cbytes, p->ept, ea);
    if (p->has_ax) {
        const QApproxBdArgs x = {approx_pass_args(g, p->member, p->flags), be};
        QG_HIP(qg_launch_approx_bd(x, st));
    } else {
        const QEltwiseBdArgs e = {g, be};
        QG_HIP(qg_launch_eltwise_bd(e, st));
    }
    return QG_OK;
}

int qgemul_time_execute_batched_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args, int warmup, int iters,
                                   float* avg_ms)
{
    if (!p || !p->has_ep) return QG_EINVAL;
    return time_execute(p, packedD, packedA, packedB, args, warmup, iters, avg_ms, TIMED_BATCHED);
}


// ---- grouped Qgemul: GEMMs of different shapes in one launch (include/qgemul.h) ----
int qgemul_classify_grouped(const qgemul_desc* d, int64_t groups, uint32_t opt_flags, qgemul_info* out)
{
    if (!d || !out) return QG_EINVAL;
    QGrouped G{};
    qgemul_info info{};
    const int st = qg_grouped_geometry(d, groups, opt_flags, &G, &info);
    if (groups >= 1) *out = info;
    return st;
}

int qgemul_classify_grouped_launches(const qgemul_desc* d, int64_t groups, uint32_t opt_flags)
{
    if (!d) return QG_EINVAL;
    QGrouped G{};
    qgemul_info info{};
    const int st = qg_grouped_geometry(d, groups, opt_flags, &G, &info);
    return st == QG_OK ? G.launches : st;
}

int qgemul_classify_grouped_member(const qgemul_desc* d, int64_t groups, uint32_t opt_flags, int64_t g, qgemul_grouped_member* out)
{
    if (!d || !out || g < 0 || g >= groups) return QG_EINVAL;
    QGrouped G{};
    qgemul_info info{};
    const int st = qg_grouped_geometry(d, groups, opt_flags, &G, &info);
    if (st == QG_OK) qg_grouped_member_out(&G, g, out);
    return st;
}

// every distinct descriptor's plain plan owns its device resources; the grouped plan owns the schedule on the device and, with a chain
// (ev), the pass form's packed C of the launch, its tile -> member table and the per-member scalar tables
static int plan_create_grouped_view(qgemul_ctx* c, const qgemul_desc* d, int64_t groups, const EpView* ev, const qgemul_grouped_ep* gep, uint32_t opt_flags,
                                    qgemul_plan** out)
{
    if (!c || !d || !out) return QG_EINVAL;
    qgemul_plan* b = new (std::nothrow) qgemul_plan();
    QGrouped* G = new (std::nothrow) QGrouped();
    int st = b && G ? qg_grouped_geometry(d, groups, opt_flags, G, &b->info, ev, gep) : QG_EINVAL;
    if (st != QG_OK) { delete G; delete b; return st; }   // (nothing on the device yet)
    b->ctx = c;
    b->grp = G;
    b->batch = -1;
    b->flags = opt_flags;
    b->desc = d[0];
    if (ev) {   // the one chain of the group (its stage kinds and containers are every member's)
        b->has_ep = 1;
        b->ep = *ev->re;
        b->ept = G->ug[G->key >= 0 ? G->key : 0].ept;
        b->has_ax = G->has_ax;
    }
    for (int64_t u = 0; u < G->n_uniq && st == QG_OK; ++u) st = plan_create_view(c, &G->ud[u], ev, opt_flags, &G->up[u], G->u_in[u] ? groups : 0);
    if (st == QG_OK) {
        DeviceScope scope(c->device);
        hipError_t e = scope.err;
        if (e == hipSuccess && G->n_tiles > 0) {
            const size_t tb = (size_t)G->n_tiles * sizeof(QGrpTile);
            e = hipMalloc((void**)&G->tiles_dev, tb);
            if (e == hipSuccess) e = hipMemcpyAsync(G->tiles_dev, G->tiles, tb, hipMemcpyHostToDevice, c->stream);
        }
        if (e == hipSuccess && G->tile_member) {   // the pass form: the launch's packed C between the two launches, and whose tile is whose
            const size_t mb = (size_t)G->n_tiles * sizeof(int32_t);
            e = hipMalloc(&G->cwork_dev, (size_t)G->launch_elems * (size_t)G->ug[G->key].pc_c.cbytes);
            if (e == hipSuccess) e = hipMalloc((void**)&G->tile_member_dev, mb);
            if (e == hipSuccess) e = hipMemcpyAsync(G->tile_member_dev, G->tile_member, mb, hipMemcpyHostToDevice, c->stream);
        }
        for (int k = 0; k < QG_MAX_EW && e == hipSuccess; ++k) {
            if (!G->per_member[k]) continue;
            G->scal[k] = new (std::nothrow) int64_t[groups]();
            if (!G->scal[k]) { st = QG_EINVAL; break; }
            e = hipMalloc((void**)&G->scal_dev[k], (size_t)groups * sizeof(int64_t));
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { g_last_hip = (int)e; st = QG_EHIP; }
    }
    if (st != QG_OK) { qgemul_plan_destroy(b); return st; }
    *out = b;
    return QG_OK;
}

int qgemul_plan_create_grouped(qgemul_ctx* c, const qgemul_desc* d, int64_t groups, uint32_t opt_flags, qgemul_plan** out)
{
    return plan_create_grouped_view(c, d, groups, nullptr, nullptr, opt_flags, out);
}

int qgemul_plan_grouped_launches(const qgemul_plan* p)
{
    if (!p || !p->grp) return QG_EINVAL;
    return p->grp->launches;
}

int qgemul_plan_grouped_member(const qgemul_plan* p, int64_t g, qgemul_grouped_member* out)
{
    if (!p || !p->grp || !out || g < 0 || g >= p->grp->groups) return QG_EINVAL;
    qg_grouped_member_out(p->grp, g, out);
    return QG_OK;
}

int qgemul_pack_grouped(qgemul_plan* p, int operand, const void* const* src_dev, const int64_t* ld, void* packed_dev)
{
    if (!p || !p->grp || !src_dev || !packed_dev || (operand != QG_OPERAND_A && operand != QG_OPERAND_B)) return QG_EINVAL;
    const QGrouped* G = p->grp;
    for (int64_t g = 0; g < G->groups; ++g) {   // every member is checked before the first launch
        const qgemul_desc& d = G->ud[G->m[g].uniq];
        if (qg_grp_empty(d)) continue;
        if (!src_dev[g] || qg_member_extent(d, operand, ld ? ld[g] : 0) < 1) return QG_EINVAL;
    }
    QG_ON_DEVICE(p->ctx);
    hipStream_t st = p->ctx->stream;
    const int check = (p->flags & QG_OPT_CHECK_RANGE) ? 1 : 0;
    const QPackedGeom& s = operand == QG_OPERAND_A ? G->sa : G->sb;
    if (G->n_in) {
        // what belongs to the launch is cleared ONCE; every member then ORs / adds into it (qg_launch_pack_stack does the same)
        if (const int rc = range_check_begin(p, check); rc != QG_OK) return rc;
        if (s.trailer) QG_HIP(hipMemsetAsync((char*)packed_dev + s.trailer, 0, QG_TRAILER_BYTES, st));
        if (s.offs && s.rows_p) QG_HIP(hipMemsetAsync((char*)packed_dev + s.rowsum_off, 0, (size_t)s.rows_p * 8, st));
        for (int64_t g = 0; g < G->groups; ++g) {
            const QGrpMember& m = G->m[g];
            if (!m.in_launch || qg_grp_empty(G->ud[m.uniq])) continue;
            const QOperandGeom og = operand_geom(G->up[m.uniq], operand, ld ? ld[g] : 0);
            QG_HIP(qg_launch_pack_member(og, operand == QG_OPERAND_A ? m.pa : m.pb, src_dev[g], (char*)packed_dev + m.off[operand], check, p->ctx->flag_dev, st,
                                         (p->flags & QG_OPT_GENERIC_LAYOUT) ? 1 : 0));
        }
        if (const int rc = range_check_end(p, check); rc != QG_OK) return rc;
    }
    for (int64_t g = 0; g < G->groups; ++g) {
        const QGrpMember& m = G->m[g];
        if (m.in_launch || qg_grp_empty(G->ud[m.uniq])) continue;
        if (const int rc = qgemul_pack(G->up[m.uniq], operand, src_dev[g], ld ? ld[g] : 0, (char*)packed_dev + m.off[operand]); rc != QG_OK) return rc;
    }
    return QG_OK;
}

int qgemul_unpack_c_grouped(qgemul_plan* p, const void* packed_dev, void* const* dst_dev, const int64_t* ld)
{
    if (!p || !p->grp || !packed_dev || !dst_dev) return QG_EINVAL;
    const QGrouped* G = p->grp;
    for (int64_t g = 0; g < G->groups; ++g) {
        const qgemul_desc& d = G->ud[G->m[g].uniq];
        if (qg_grp_empty(d)) continue;
        if (!dst_dev[g] || qg_member_extent(d, QG_OPERAND_C, ld ? ld[g] : 0) < 1) return QG_EINVAL;
    }
    for (int64_t g = 0; g < G->groups; ++g) {   // (a layout step: one launch per member)
        const QGrpMember& m = G->m[g];
        if (qg_grp_empty(G->ud[m.uniq])) continue;
        if (const int rc = qgemul_unpack_c(G->up[m.uniq], (const char*)packed_dev + m.off[2], dst_dev[g], ld ? ld[g] : 0); rc != QG_OK) return rc;
    }
    return QG_OK;
}

// the grouped launch's uniform arguments (what every workgroup shares: the launch key's variant and conversion into C, the stacks'
// plane masks and row sums) and the schedule; cbytes: the container the kernel stores
static QMfmaGrpArgs grp_mfma_args(const QGrouped* G, void* packedC, const void* packedA, const void* packedB, int cbytes)
{
    const QPlanGeom& k = G->ug[G->key];
    QMfmaGrpArgs a;
    memset((void*)&a, 0, sizeof a);
    (QMfmaArgs&)a = mfma_args(G->sa, G->sb, k.variant, packedA, packedB, packedC, cbytes);
    a.to_c = k.an.lin.to_c[0];
    centre_args(a, G->sa, G->sb, packedA, packedB, 0);
    a.tiles = G->tiles_dev;
    return a;
}

int qgemul_execute_grouped(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB)
{
    if (!p || !p->grp || !packedC || !packedA || !packedB) return QG_EINVAL;
    const QGrouped* G = p->grp;
    if (G->has_ep) return QG_EINVAL;   // a grouped plan with a chain runs through qgemul_execute_grouped_ep
    if (G->n_tiles > 0) {
        QG_ON_DEVICE(p->ctx);
        const QPlanGeom& k = G->ug[G->key];
        QG_HIP(qg_launch_mfma_grp(k.LA, k.LB, grp_mfma_args(G, packedC, packedA, packedB, k.pc.cbytes), G->n_tiles, p->ctx->stream));
    }
    for (int64_t g = 0; g < G->groups; ++g) {
        const QGrpMember& m = G->m[g];
        if (m.in_launch) continue;
        if (const int rc = qgemul_execute(G->up[m.uniq], (char*)packedC + m.off[2], (const char*)packedA + m.off[0], (const char*)packedB + m.off[1]); rc != QG_OK)
            return rc;
    }
    return QG_OK;
}

int qgemul_time_execute_grouped(qgemul_plan* p, void* packedC, const void* packedA, const void* packedB, int warmup, int iters, float* avg_ms)
{
    return time_execute(p, packedC, packedA, packedB, nullptr, warmup, iters, avg_ms, TIMED_GROUPED);
}

// ---- element-wise chains on grouped plans (include/qgemul.h): member g is Qgemul<...>(C_g, A_g, B_g) followed by the chain ----
static int grouped_ep_geometry(const qgemul_desc* d, int64_t groups, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW], const qgemul_grouped_ep* gep,
                               uint32_t opt_flags, QGrouped* G, qgemul_info* info)
{
    if (!d || !ep) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax ? ax : g_no_ax};
    return qg_grouped_geometry(d, groups, opt_flags, G, info, &v, gep);
}

int qgemul_classify_grouped_epx(const qgemul_desc* d, int64_t groups, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                const qgemul_grouped_ep* gep, uint32_t opt_flags, qgemul_info* out)
{
    if (!out) return QG_EINVAL;
    QGrouped G{};
    qgemul_info info{};
    const int st = grouped_ep_geometry(d, groups, ep, ax, gep, opt_flags, &G, &info);
    if (d && ep && groups >= 1) *out = info;
    return st;
}

int qgemul_classify_grouped_epx_launches(const qgemul_desc* d, int64_t groups, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                         const qgemul_grouped_ep* gep, uint32_t opt_flags)
{
    QGrouped G{};
    qgemul_info info{};
    const int st = grouped_ep_geometry(d, groups, ep, ax, gep, opt_flags, &G, &info);
    return st == QG_OK ? G.launches : st;
}

int qgemul_classify_grouped_epx_member(const qgemul_desc* d, int64_t groups, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                       const qgemul_grouped_ep* gep, uint32_t opt_flags, int64_t g, qgemul_grouped_member* out)
{
    if (!out || g < 0 || g >= groups) return QG_EINVAL;
    QGrouped G{};
    qgemul_info info{};
    const int st = grouped_ep_geometry(d, groups, ep, ax, gep, opt_flags, &G, &info);
    if (st == QG_OK) qg_grouped_member_out(&G, g, out);
    return st;
}

int qgemul_plan_create_grouped_epx(qgemul_ctx* c, const qgemul_desc* d, int64_t groups, const qgemul_epilogue* ep, const qgemul_approx* const ax[QG_MAX_EW],
                                   const qgemul_grouped_ep* gep, uint32_t opt_flags, qgemul_plan** out)
{
    if (!c || !d || !ep || !out) return QG_EINVAL;
    const EpView v = {ep, nullptr, nullptr, ax ? ax : g_no_ax};
    return plan_create_grouped_view(c, d, groups, &v, gep, opt_flags, out);
}

// per-member values are model constants: the host copy serves the stragglers, the device table the launch; the upload has ended when
// this returns, so every later execute sees the new values
int qgemul_grouped_set_scalars(qgemul_plan* p, int stage, const int64_t* host_values)
{
    if (!p || !p->grp || !p->grp->has_ep || !host_values || stage < 0 || stage >= p->ept.n || !p->grp->per_member[stage]) return QG_EINVAL;
    QGrouped* G = p->grp;
    QG_ON_DEVICE(p->ctx);
    // (an execute queued earlier may still read the table: the copy is ordered behind it on the stream, and its source is the plan's)
    QG_HIP(hipStreamSynchronize(p->ctx->stream));
    memcpy(G->scal[stage], host_values, (size_t)G->groups * sizeof(int64_t));
    QG_HIP(hipMemcpyAsync(G->scal_dev[stage], G->scal[stage], (size_t)G->groups * sizeof(int64_t), hipMemcpyHostToDevice, p->ctx->stream));
    QG_HIP(hipStreamSynchronize(p->ctx->stream));
    G->scal_set[stage] = 1;
    return QG_OK;
}

int qgemul_pack_e_grouped(qgemul_plan* p, int stage, const void* const* src_dev, const int64_t* ld, void* packed_dev)
{
    if (!p || !p->grp || !p->grp->has_ep || !src_dev || !packed_dev || stage < 0 || stage >= p->ept.n) return QG_EINVAL;
    const QGrouped* G = p->grp;
    if (p->ept.st[stage].scalar) return QG_EINVAL;   // a scalar or APPROX stage has no tensor operand
    for (int64_t g = 0; g < G->groups; ++g) {   // every member is checked before the first launch
        const qgemul_desc& d = G->ud[G->m[g].uniq];
        if (qg_grp_empty(d)) continue;
        if (!src_dev[g] || qg_member_extent(d, QG_OPERAND_C, ld ? ld[g] : 0) < 1) return QG_EINVAL;
    }
    for (int64_t g = 0; g < G->groups; ++g) {   // (a layout step: one launch per member)
        const QGrpMember& m = G->m[g];
        if (qg_grp_empty(G->ud[m.uniq])) continue;
        if (const int rc = qgemul_pack_e(G->up[m.uniq], stage, src_dev[g], ld ? ld[g] : 0, (char*)packed_dev + m.eoff[stage]); rc != QG_OK) return rc;
    }
    return QG_OK;
}

int qgemul_execute_grouped_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args)
{
    if (!p || !p->grp || !p->grp->has_ep || !packedD || !packedA || !packedB) return QG_EINVAL;
    const QGrouped* G = p->grp;
    if (int s = ep_args_ok(p, args)) return s;
    for (int k = 0; k < p->ept.n; ++k)
        if (G->per_member[k] && !G->scal_set[k]) return QG_EINVAL;   // qgemul_grouped_set_scalars has not filled the stage's table
    if (G->n_tiles > 0) {
        QG_ON_DEVICE(p->ctx);
        hipStream_t st = p->ctx->stream;
        const QPlanGeom& k = G->ug[G->key];
        const QEpArgs ea = ep_device_args(p, args);
        QGrpEp ge;
        memset(&ge, 0, sizeof ge);
        for (int s = 0; s < p->ept.n; ++s)
            if (G->per_member[s]) ge.scal[s] = G->scal_dev[s];
        // the launch's uniform arguments: those of qgemul_execute_grouped, with the kernel's own C container
        const QMfmaGrpArgs a = grp_mfma_args(G, G->fused ? packedD : G->cwork_dev, packedA, packedB, k.pc_c.cbytes);
        if (G->fused) {
            // ONE launch: the grouped kernel's epilogue runs the chain on the value it has just converted into C's type
            QMfmaEpGrpArgs f;
            memset((void*)&f, 0, sizeof f);
            (QMfmaArgs&)f = a;
            f.tiles = a.tiles;
            f.has_ep = 1;
            f.ep = k.ept;
            f.epa = ea;
            f.ge = ge;
            QG_HIP(qg_launch_mfma_ep_grp(k.LA, k.LB, f, G->n_tiles, st));
        } else {
            // TWO launches: the grouped kernel as it is into the plan's packed C of the launch, then ONE pass over its tiles into D
            QG_HIP(qg_launch_mfma_grp(k.LA, k.LB, a, G->n_tiles, st));
            const QEltwiseArgs g = chain_pass_args(G->cwork_dev, packedD, G->launch_elems, k.pc_c.cbytes, k.ept, ea);
            if (G->has_ax) {
                const QApproxGrpArgs x = {approx_pass_args(g, G->up[G->key], p->flags), G->tile_member_dev, ge};
                QG_HIP(qg_launch_approx_grp(x, st));
            } else {
                const QEltwiseGrpArgs e = {g, G->tile_member_dev, ge};
                QG_HIP(qg_launch_eltwise_grp(e, st));
            }
        }
    }
    // the stragglers: their own plain _epx plans, with the member's scalars and its part of every packed tensor operand
    for (int64_t g = 0; g < G->groups; ++g) {
        const QGrpMember& m = G->m[g];
        if (m.in_launch) continue;
        qgemul_ep_args ma;
        memset(&ma, 0, sizeof ma);
        for (int k = 0; k < p->ept.n; ++k) {
            ma.e_scalar[k] = G->per_member[k] ? G->scal[k][g] : args->e_scalar[k];
            if (!p->ept.st[k].scalar) ma.e_packed[k] = (const char*)args->e_packed[k] + m.eoff[k];
        }
        if (const int rc = qgemul_execute_ep(G->up[m.uniq], (char*)packedD + m.off[2], (const char*)packedA + m.off[0], (const char*)packedB + m.off[1], &ma); rc != QG_OK)
            return rc;
    }
    return QG_OK;
}

int qgemul_time_execute_grouped_ep(qgemul_plan* p, void* packedD, const void* packedA, const void* packedB, const qgemul_ep_args* args, int warmup, int iters,
                                   float* avg_ms)
{
    if (!p || !p->grp || !p->grp->has_ep) return QG_EINVAL;
    return time_execute(p, packedD, packedA, packedB, args, warmup, iters, avg_ms, TIMED_GROUPED_EP);
}

} // extern "C"
