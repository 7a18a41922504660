// qg_run_key.h — what identifies the plan a one-shot call (qgemul_run*, qg_run.hip) keeps between two calls.  Host code without
// HIP types: a host compiler builds it alone (tests/san/run_key_driver.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/qgemul.h"

#pragma GCC visibility push(hidden)   // internal to the library: nothing here is an exported symbol

// an element-wise chain as the planner sees it: a real chain (im == nullptr) or the two part chains of a complex one
struct EpView { const qgemul_epilogue* re; const qgemul_epilogue* im; const uint8_t* e_cplx; const qgemul_approx* const* ax; const qgemul_epilogue_cplx* epc; const qgemul_cmul* const* cx; };

// The key of a cached plan: every input the plan was made from.  The setters write EVERY field — what a request does not have is
// written as zero / off —, so no field keeps an earlier plan's value, and qg_run_key_equal needs no knowledge of which entry point
// stored the key.  The tables of APPROX stages (2.3 KB each) and a grouped request's descriptor list live on the heap, present only
// while a stage carries a table / the request is a grouped one.
struct QRunKey {
    qgemul_desc d;                    // the plain or batched request's descriptor (a grouped request: zero, its descriptors are `member`)
    uint32_t flags;
    int64_t batch;                    // 0: not a batched plan; > 0: a batched plan of that many members
    int64_t groups;                   // 0: not a grouped plan; > 0: a grouped plan of that many members
    qgemul_desc* member;              // the group's descriptors in list order: `groups` entries, allocated while groups > 0
    uint8_t has_ep, ep_cplx;          // a chain; ... of a complex GEMM (both part chains)
    qgemul_epilogue part[2];          // a real chain is part[0]
    uint8_t e_complex[QG_MAX_EW];
    uint8_t ax_on[QG_MAX_EW];         // stage k carries an APPROX table: ax[k]
    qgemul_approx* ax;                // QG_MAX_EW tables, allocated while any ax_on[k]
    uint8_t cx_on[QG_MAX_EW];         // stage k carries a CMUL record: cx[k]
    qgemul_cmul cx[QG_MAX_EW];
    uint8_t e_shared[QG_MAX_EW];            // batched chain: stage k's tensor operand is one tensor for every member
    uint8_t scalar_per_member[QG_MAX_EW];   // grouped chain: scalar stage k takes one value per member

    QRunKey() { memset((void*)this, 0, sizeof *this); }
    QRunKey(const QRunKey& o) : QRunKey() { *this = o; }
    ~QRunKey() { delete[] ax; delete[] member; }
    QRunKey& operator=(const QRunKey& o)
    {
        if (this == &o) return *this;
        const Heap mine = heap();
        memcpy((void*)this, (const void*)&o, sizeof *this);
        keep(mine);
        const qgemul_approx* from[QG_MAX_EW];
        for (int k = 0; k < QG_MAX_EW; ++k) from[k] = ax_on[k] ? &o.ax[k] : nullptr;
        tables(from);
        members(o.member, o.groups);
        return *this;
    }
    // what this key owns on the heap, carried over a memset / memcpy of the whole object (groups: the length `member` is allocated at)
    struct Heap { qgemul_approx* ax; qgemul_desc* member; int64_t groups; };
    Heap heap() const { return {ax, member, groups}; }
    void keep(const Heap& h) { ax = h.ax; member = h.member; groups = h.groups; }
    // this key's own copy of the tables that ax_on names (none: no allocation)
    void tables(const qgemul_approx* const* from)
    {
        bool any = false;
        for (int k = 0; k < QG_MAX_EW; ++k) any = any || ax_on[k];
        if (!any) { delete[] ax; ax = nullptr; return; }
        if (!ax) ax = new qgemul_approx[QG_MAX_EW];
        for (int k = 0; k < QG_MAX_EW; ++k)
            if (ax_on[k]) ax[k] = *from[k];
    }
    // this key's own copy of a group's n descriptors (n == 0, a request that is not grouped: no allocation)
    void members(const qgemul_desc* from, int64_t n)
    {
        if (n != groups) {
            delete[] member;
            member = nullptr;   // (the key stays whole if the allocation throws)
            groups = 0;
            if (n) member = new qgemul_desc[n];
            groups = n;
        }
        for (int64_t g = 0; g < n; ++g) member[g] = from[g];
    }
};

// The one body of the two setters below.  d: `groups` descriptors of a grouped request, one otherwise (groups == 0)
inline void qg_run_key_write(QRunKey& key, const qgemul_desc* d, int64_t groups, uint32_t flags, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep,
                             const qgemul_grouped_ep* gep)
{
    const QRunKey::Heap mine = key.heap();
    memset((void*)&key, 0, sizeof key);
    key.keep(mine);
    if (!groups) key.d = *d;
    key.members(d, groups);
    key.flags = flags;
    key.batch = batch;
    if (ev) {
        key.has_ep = 1;
        key.part[0] = *ev->re;
        if (ev->im) {
            key.ep_cplx = 1;
            key.part[1] = *ev->im;
            for (uint32_t k = 0; k < ev->re->n_stages && k < QG_MAX_EW; ++k) key.e_complex[k] = ev->e_cplx[k];
        }
        for (int k = 0; k < QG_MAX_EW; ++k) {
            key.ax_on[k] = ev->ax && ev->ax[k];
            if (ev->cx && ev->cx[k]) { key.cx_on[k] = 1; key.cx[k] = *ev->cx[k]; }
        }
    }
    key.tables(ev ? ev->ax : nullptr);
    if (bep) memcpy(key.e_shared, bep->e_shared, sizeof key.e_shared);
    if (gep) memcpy(key.scalar_per_member, gep->scalar_per_member, sizeof key.scalar_per_member);
}

// a plain (batch == 0) or batched request.  ev: the chain (nullptr: none); bep: which tensor operands of a batched chain are shared (nullptr: none)
inline void qg_run_key_set(QRunKey& key, const qgemul_desc& d, uint32_t flags, int64_t batch, const EpView* ev, const qgemul_batched_ep* bep)
{
    qg_run_key_write(key, &d, 0, flags, batch, ev, bep, nullptr);
}
// a grouped request of groups >= 1 members.  ev: the group's one chain (nullptr: none); gep: which of its scalar stages take a value per member (nullptr: none)
inline void qg_run_key_set_grouped(QRunKey& key, const qgemul_desc* d, int64_t groups, uint32_t flags, const EpView* ev, const qgemul_grouped_ep* gep)
{
    qg_run_key_write(key, d, groups, flags, 0, ev, nullptr, gep);
}

// Field by field: padding and reserved bytes of a caller's struct are not part of its meaning, and a descriptor that was not built
// with `{}` must still hit the cache; only n_levels / n_stages / n_seg / n_coef entries count.
inline bool same_fmt(const qfmt& x, const qfmt& y) { return x.I == y.I && x.F == y.F && x.S == y.S && x.Q == y.Q && x.O == y.O; }
inline bool same_desc(const qgemul_desc& x, const qgemul_desc& y)
{
    if (x.abi != y.abi || x.transA != y.transA || x.is_complex != y.is_complex || x.cmul != y.cmul || x.flags != y.flags || x.M != y.M || x.N != y.N ||
        x.K != y.K || x.n_levels != y.n_levels || x.n_levels > QG_MAX_LEVELS)
        return false;
    for (int p = 0; p < 2; ++p) {
        if (!same_fmt(x.a[p], y.a[p]) || !same_fmt(x.b[p], y.b[p]) || !same_fmt(x.c[p], y.c[p])) return false;
        for (uint32_t l = 0; l < x.n_levels; ++l)
            if (!same_fmt(x.level_add[p][l], y.level_add[p][l]) || !same_fmt(x.level[p][l], y.level[p][l])) return false;
    }
    for (int i = 0; i < 8; ++i)
        if (!same_fmt(x.mul[i], y.mul[i])) return false;
    return true;
}
inline bool same_epilogue(const qgemul_epilogue& x, const qgemul_epilogue& y)
{
    if (x.n_stages != y.n_stages || x.n_stages > QG_MAX_EW || !same_fmt(x.d, y.d)) return false;
    for (uint32_t k = 0; k < x.n_stages; ++k) {
        const qgemul_ew_stage &a = x.stage[k], &b = y.stage[k];
        if (a.op != b.op || a.x_first != b.x_first || a.e_scalar != b.e_scalar || !same_fmt(a.e, b.e) || !same_fmt(a.r, b.r) || !same_fmt(a.t, b.t))
            return false;
    }
    return true;
}
inline bool same_approx(const qgemul_approx& x, const qgemul_approx& y)
{
    if (x.n_seg != y.n_seg || x.n_seg > QG_MAX_SEG) return false;
    for (uint32_t g = 0; g < x.n_seg; ++g) {
        const qgemul_approx_seg &a = x.seg[g], &b = y.seg[g];
        if (memcmp(&a.breakpoint, &b.breakpoint, sizeof a.breakpoint) || a.n_coef != b.n_coef || a.n_coef > QG_MAX_COEF) return false;
        for (uint32_t i = 0; i < a.n_coef; ++i)
            if (!same_fmt(a.f[i], b.f[i]) || a.a[i] != b.a[i]) return false;
    }
    return true;
}
inline bool same_cmul(const qgemul_cmul& x, const qgemul_cmul& y)
{
    if (x.cmul != y.cmul) return false;
    for (int i = 0; i < 8; ++i)
        if (!same_fmt(x.mul[i], y.mul[i])) return false;
    return true;
}

inline bool qg_run_key_equal(const QRunKey& x, const QRunKey& y)
{
    if (x.flags != y.flags || x.batch != y.batch || x.groups != y.groups || x.has_ep != y.has_ep || x.ep_cplx != y.ep_cplx || !same_desc(x.d, y.d)) return false;
    for (int64_t g = 0; g < x.groups; ++g)
        if (!same_desc(x.member[g], y.member[g])) return false;
    if (x.has_ep && !same_epilogue(x.part[0], y.part[0])) return false;
    if (x.ep_cplx && (!same_epilogue(x.part[1], y.part[1]) || memcmp(x.e_complex, y.e_complex, sizeof x.e_complex))) return false;
    for (int k = 0; k < QG_MAX_EW; ++k) {
        if (x.ax_on[k] != y.ax_on[k] || x.cx_on[k] != y.cx_on[k]) return false;
        if (x.ax_on[k] && !same_approx(x.ax[k], y.ax[k])) return false;
        if (x.cx_on[k] && !same_cmul(x.cx[k], y.cx[k])) return false;
    }
    return !memcmp(x.e_shared, y.e_shared, sizeof x.e_shared) && !memcmp(x.scalar_per_member, y.scalar_per_member, sizeof x.scalar_per_member);
}

#pragma GCC visibility pop
