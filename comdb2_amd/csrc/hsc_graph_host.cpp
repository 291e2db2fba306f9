// hsc_graph_host.cpp -- host side of the dependency-graph entries
// (hsc_dep_graph_*): upload or take a history's ops, build the graph, and run
// the SCC / anomaly / SI / resolve passes of hsc_graph.hip and its neighbours
// on the context's stream.  Reaches the context only through hsc_ctx.h; the
// window's own entries (hsc_rw_edges among them) are in hsc_host.cpp.
#include "hsc_ctx.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

// An entry's way in, after its argument checks: a host-only context has no
// device; else the context's lock, then its device.
#define GRAPH_ENTRY(c)                      \
    if ((c)->host_only) return HSC_EDEVICE; \
    MuGuard g_(c);                          \
    (void)hipSetDevice((c)->device)

// (never a null array: an empty vector's data() may be)
static const uint64_t kZeros[2] = {0, 0};
template <class T>
static const T *data_or_zero(const std::vector<T> &v)
{
    return v.empty() ? (const T *)kZeros : v.data();
}

// Build c->graph from device-resident ops (edges and CSR/CSC), timed with
// events.  Caller holds c->mu.
static int graph_build_timed(hsc_ctx *c, const GraphInput &in, bool full, float *build_ms)
{
    hipStream_t s = c->stream;
    GraphBufs &gb = c->graph;
    EventSpan t;
    HIPCHK(c, t.begin(s));
    GraphInput gi = in;
    // staged rows that would index past the CSR arrays, or the real-time order
    // of another history: the build fails and every staged edge is dropped
    const bool bad_rw = gb.n_extra && c->x_max_txn >= in.ntxn;
    const bool bad_rt = gb.rt_staged && gb.rt_ntxn != in.ntxn;
    if (bad_rw || bad_rt) {
        gb.n_extra = 0;
        gb.rt_staged = false;
        gb.n_rt = 0;
        return ctx_fail(c, HSC_EINVAL, bad_rw ? "a staged rw pair names a txn >= the build's ntxn"
                                              : "the staged real-time order is of another ntxn than the build's");
    }
    if (gb.n_extra) {  // staged edges join this build, once
        gi.x_rows = gb.x_rows.as<uint64_t>();
        gi.x_type = gb.x_type.as<uint64_t>();
        gi.n_extra = gb.n_extra;
        gb.n_extra = 0;
    }
    if (gb.rt_staged) {  // and the staged real-time order, a segment of its own
        gi.r_rows = gb.rt_rows.as<uint64_t>();
        gi.r_type = gb.rt_type.as<uint64_t>();
        gi.n_rt = gb.n_rt;
        gb.rt_staged = false;
        gb.n_rt = 0;
    }
    gb.edge_bad = nullptr;
    gb.post = nullptr;
    HIPCHK(c, graph_build(gi, gb, full, s));
    HIPCHK(c, t.end(s));
    // with the sync: the backward rows listed and the edge pass's check of the
    // observed ids (in.check)
    uint32_t post[3] = {0, 0, 0};
    if (gb.post) HIPCHK(c, hipMemcpyAsync(post, gb.post - 1, 12, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *build_ms = t.ms();
    if (post[0] && gb.writer_packed) return ctx_fail(c, HSC_EDEVICE, "graph build: the writer sort's look-back stalled");
    gb.back_n = post[1];
    const uint32_t ebad = gb.edge_bad ? post[2] : 0;
    gb.bad |= ebad;
    if (ebad & 1) {
        c->graph_ntxn = 0;
        return ctx_fail(c, HSC_EINVAL, "history op out of range");
    }
    c->graph_ntxn = in.ntxn;
    return HSC_OK;
}

// Upload a history and build its graph into c->graph (edges and CSR/CSC).
// Caller holds c->mu.
static int graph_upload_build(hsc_ctx *c, const hsc_history *h, bool full, float *build_ms,
                              bool skip_rw = false)
{
    if (!h || (h->nops && (!h->txn || !h->key || !h->is_write || !h->observed)) ||
        h->nops > 0x7FFFFFFFull)
        return HSC_EINVAL;
    if (c->host_only) return ctx_fail(c, HSC_EDEVICE, "host-only context");
    (void)hipSetDevice(c->device);
    for (size_t i = 0; i < h->nops; ++i)
        if (h->txn[i] >= h->ntxn || h->observed[i] >= (int64_t)h->ntxn || h->observed[i] < -1)
            return ctx_fail(c, HSC_EINVAL, "history op out of range");
    hipStream_t s = c->stream;
    GraphBufs &gb = c->graph;
    const size_t n = h->nops;
    std::vector<uint32_t> obs(std::max<size_t>(n, 1));
    for (size_t i = 0; i < n; ++i) obs[i] = h->observed[i] < 0 ? 0xFFFFFFFFu : (uint32_t)h->observed[i];
    HIPCHK(c, gb.h_txn.ensure(4 * std::max<size_t>(n, 1)));
    HIPCHK(c, gb.h_key.ensure(8 * std::max<size_t>(n, 1)));
    HIPCHK(c, gb.h_isw.ensure(std::max<size_t>(n, 1)));
    HIPCHK(c, gb.h_obs.ensure(4 * std::max<size_t>(n, 1)));
    if (n) {
        HIPCHK(c, hipMemcpyAsync(gb.h_txn.p, h->txn, 4 * n, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(gb.h_key.p, h->key, 8 * n, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(gb.h_isw.p, h->is_write, n, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(gb.h_obs.p, obs.data(), 4 * n, hipMemcpyHostToDevice, s));
    }
    GraphInput in{gb.h_txn.as<uint32_t>(), gb.h_key.as<uint64_t>(), gb.h_isw.as<uint8_t>(),
                  gb.h_obs.as<uint32_t>(), n, h->ntxn};
    in.skip_rw = skip_rw;
    return graph_build_timed(c, in, full, build_ms);
}

// Edge and edge-type counts of c->graph into st (none after a raw build).
static int graph_edge_stats(hsc_ctx *c, hsc_graph_stats *st)
{
    GraphBufs &gb = c->graph;
    st->edges = gb.ne;
    uint64_t t[3] = {0, 0, 0};
    HIPCHK(c, graph_type_counts(gb, t, c->stream));
    st->ww = t[0];
    st->wr = t[1];
    st->rw = t[2];
    return HSC_OK;
}

// The end of a build entry: rc of the build; its time and the edge counts
// into st where the caller asked for them.
static int build_stats(hsc_ctx *c, int rc, float build_ms, hsc_graph_stats *st)
{
    if (rc || !st) return rc;
    memset(st, 0, sizeof *st);
    st->build_ms = build_ms;
    return graph_edge_stats(c, st);
}

static void scc_size_stats(const uint32_t *scc, uint32_t ntxn, hsc_graph_stats *st)
{
    std::vector<uint32_t> sz(std::max<uint32_t>(ntxn, 1), 0);
    for (uint32_t v = 0; v < ntxn; ++v)
        if (scc[v] < ntxn) sz[scc[v]]++;
    for (uint32_t v = 0; v < ntxn; ++v)
        if (sz[v] > 1) {
            st->nontrivial_sccs++;
            st->txns_in_cycles += sz[v];
        }
}

// The components of c->graph's nn txns, timed: the colours into scc_out, the
// counts into st (its build_ms stays 0).  Caller holds c->mu.
static int scc_timed(hsc_ctx *c, uint32_t nn, uint32_t *scc_out, hsc_graph_stats *st)
{
    hipStream_t s = c->stream;
    GraphBufs &gb = c->graph;
    EventSpan t;
    HIPCHK(c, t.begin(s));
    uint32_t rounds = 0, iters = 0;
    HIPCHK(c, graph_scc(nn, gb, &rounds, &iters, s));
    HIPCHK(c, t.end(s));
    if (nn) HIPCHK(c, hipMemcpyAsync(scc_out, gb.scc.p, 4 * (size_t)nn, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (!st) return HSC_OK;
    memset(st, 0, sizeof *st);
    st->scc_ms = t.ms();
    HIPCHK_RC(c, graph_edge_stats(c, st));
    scc_size_stats(scc_out, nn, st);
    st->rounds = rounds;
    st->iterations = iters;
    return HSC_OK;
}

extern "C" {

int hsc_dep_graph_scc(hsc_ctx *c, const hsc_history *h, uint32_t *scc_out, hsc_graph_stats *st)
{
    if (!c || !h || (h->ntxn && !scc_out)) return HSC_EINVAL;
    MuGuard g(c);
    float build_ms = 0;
    HIPCHK_RC(c, graph_upload_build(c, h, true, &build_ms));
    const int rc = scc_timed(c, h->ntxn, scc_out, st);
    if (rc == HSC_OK && st) st->build_ms = build_ms;
    return rc;
}

int hsc_dep_graph_build(hsc_ctx *c, const hsc_history *h, int flags, hsc_graph_stats *st)
{
    if (!c || !h) return HSC_EINVAL;
    MuGuard g(c);
    float build_ms = 0;
    const int rc = graph_upload_build(c, h, (flags & HSC_GRAPH_FULL) != 0, &build_ms,
                                      (flags & HSC_GRAPH_NO_RW) != 0);
    return build_stats(c, rc, build_ms, st);
}

int hsc_dep_graph_build_device(hsc_ctx *c, size_t nops, uint32_t ntxn, const uint32_t *txn_dev,
                               const uint64_t *key_dev, const uint8_t *is_write_dev,
                               const uint32_t *observed_dev, int flags, hsc_graph_stats *st)
{
    if (!c || (nops && (!txn_dev || !key_dev || !is_write_dev || !observed_dev)) ||
        nops > 0x7FFFFFFFull)
        return HSC_EINVAL;
    GRAPH_ENTRY(c);
    GraphInput in{txn_dev, key_dev, is_write_dev, observed_dev, nops, ntxn};
    in.skip_rw = (flags & HSC_GRAPH_NO_RW) != 0;
    in.check = true;  // the ids and the txn order, in the build's first pass
    float build_ms = 0;
    const int rc = graph_build_timed(c, in, (flags & HSC_GRAPH_FULL) != 0, &build_ms);
    if (rc && (c->graph.bad & 1)) return ctx_fail(c, HSC_EINVAL, "history op out of range");
    return build_stats(c, rc, build_ms, st);
}

int hsc_dep_graph_resolve(hsc_ctx *c, const hsc_vhistory *h, unsigned flags, hsc_resolved *out)
{
    if (!c || !h || !out || (h->nops && (!h->txn || !h->key || !h->is_write || !h->value)) ||
        (h->ntxn && !h->status) || h->nops > 0x7FFFFFFFull || h->ntxn > 0x7FFFFFFFu)
        return HSC_EINVAL;
    GRAPH_ENTRY(c);
    hipStream_t s = c->stream;
    static const int dir_bits = [] {  // (A/B diagnostics: 0 = the plain binary search)
        const char *v = getenv("HSC_RESOLVE_DIR_BITS");
        return v ? atoi(v) : -1;
    }();
    EventSpan t;
    ResolveOut &o = c->resolve_out;
    const ResolveIn in{h->nops, h->ntxn, h->txn, h->key, h->is_write, h->value, h->status};
    hipError_t e = t.begin(s);
    if (e == hipSuccess) e = graph_resolve(in, c->resolve, (flags & HSC_RESOLVE_ARRAYS) != 0, dir_bits, o, s);
    const int bad = o.bad;
    if (e == hipSuccess) e = t.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    memset(out, 0, sizeof *out);
    if (e == hipErrorInvalidValue && bad)
        return ctx_fail(c, HSC_EINVAL,
                        bad & 1   ? "value history: an op names a txn >= ntxn"
                        : bad & 2 ? "value history: a write of HSC_VAL_INIT"
                        : bad & 4 ? "value history: a status above HSC_TXN_UNKNOWN"
                                  : "value history: a written (key, value) occurs twice");
    HIPCHK(c, e);
    out->ms = t.ms();
    out->nops = h->nops;
    out->kept_ops = o.kept_ops;
    out->ntxn = h->ntxn;
    out->ncommitted = o.ncommitted;
    out->recovered = o.recovered;
    out->aborted = o.aborted;
    out->dropped = o.dropped;
    out->writes = o.writes;
    out->reads = o.reads;
    out->g1a_reads = o.g1a_reads;
    out->g1b_reads = o.g1b_reads;
    out->dangling_reads = o.dangling_reads;
    out->internal_reads = o.internal_reads;
    out->g1a_txns = o.g1a_txns;
    out->g1b_txns = o.g1b_txns;
    out->fate = data_or_zero(o.fate);
    out->cid = data_or_zero(o.cid);
    out->txn_of_cid = data_or_zero(o.txn_of_cid);
    out->txn_g1 = data_or_zero(o.txn_g1);
    out->n_listed = o.n_listed;
    out->listed_op = data_or_zero(o.listed_op);
    out->listed_wop = data_or_zero(o.listed_wop);
    if (flags & HSC_RESOLVE_ARRAYS) {
        out->obs_txn = data_or_zero(o.obs_txn);
        out->obs_op = data_or_zero(o.obs_op);
        out->rflag = data_or_zero(o.rflag);
    }
    out->sweeps = o.sweeps;
    return HSC_OK;
}

int hsc_dep_graph_build_resolved(hsc_ctx *c, int flags, hsc_graph_stats *st)
{
    if (!c) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    const ResolveBufs &r = c->resolve;
    if (!r.valid) return ctx_fail(c, HSC_ESTATE, "no resolved history (hsc_dep_graph_resolve)");
    GraphInput in{r.l_txn.as<uint32_t>(), r.l_key.as<uint64_t>(), r.l_isw.as<uint8_t>(), r.l_obs.as<uint32_t>(),
                  r.kept, r.nc};
    in.skip_rw = (flags & HSC_GRAPH_NO_RW) != 0;
    in.check = true;  // finds whether the kept ops are in txn order
    float build_ms = 0;
    const int rc = graph_build_timed(c, in, (flags & HSC_GRAPH_FULL) != 0, &build_ms);
    return build_stats(c, rc, build_ms, st);
}

int hsc_dep_graph_resolve_sort_path(hsc_ctx *c) { return c ? c->resolve.sort_path : 0; }

int hsc_dep_graph_resolve_lists(hsc_ctx *c, const hsc_lhistory *h, unsigned flags, hsc_lresolved *out)
{
    if (!c || !h || !out || (h->nops && (!h->txn || !h->key || !h->is_write || !h->value || !h->list_off)) ||
        (h->ntxn && !h->status) || h->nops > 0x7FFFFFFFull || h->ntxn > 0x7FFFFFFFu)
        return HSC_EINVAL;
    const uint64_t ne = h->nops ? h->list_off[h->nops] : 0;
    if (ne > 0x7FFFFFFFull || (ne && !h->elems)) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    hipStream_t s = c->stream;
    EventSpan t;
    ListOut &o = c->lists_out;
    const ListIn in{h->nops, h->ntxn, h->txn, h->key, h->is_write, h->value, h->list_off, h->elems, h->status};
    hipError_t e = t.begin(s);
    if (e == hipSuccess) e = graph_resolve_lists(in, c->lists, (flags & HSC_RESOLVE_ARRAYS) != 0, o, s);
    const int bad = o.bad;
    if (e == hipSuccess) e = t.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    memset(out, 0, sizeof *out);
    if (e == hipErrorInvalidValue && bad)
        return ctx_fail(c, HSC_EINVAL,
                        bad & 1   ? "list history: an op names a txn >= ntxn"
                        : bad & 2 ? "list history: list_off is not ascending"
                        : bad & 4 ? "list history: a status above HSC_TXN_UNKNOWN"
                                  : "list history: an appended (key, element) occurs twice");
    HIPCHK(c, e);
    out->ms = t.ms();
    out->nops = h->nops;
    out->ntxn = h->ntxn;
    out->ncommitted = o.ncommitted;
    out->recovered = o.recovered;
    out->aborted = o.aborted;
    out->dropped = o.dropped;
    out->appends = o.appends;
    out->reads = o.reads;
    out->elements = o.elements;
    out->keys = o.keys;
    out->incompatible_keys = o.incompatible_keys;
    out->spine_elements = o.spine_elements;
    out->chain_entries = o.chain_entries;
    out->ww = o.ww;
    out->wr = o.wr;
    out->rw = o.rw;
    out->g1a_reads = o.g1a_reads;
    out->g1b_reads = o.g1b_reads;
    out->dangling_reads = o.dangling_reads;
    out->duplicate_reads = o.duplicate_reads;
    out->incompatible_reads = o.incompatible_reads;
    out->internal_reads = o.internal_reads;
    out->unobserved_appends = o.unobserved_appends;
    out->g1a_txns = o.g1a_txns;
    out->g1b_txns = o.g1b_txns;
    out->fate = data_or_zero(o.fate);
    out->cid = data_or_zero(o.cid);
    out->txn_of_cid = data_or_zero(o.txn_of_cid);
    out->txn_g1 = data_or_zero(o.txn_g1);
    out->n_listed = o.n_listed;
    out->listed_op = data_or_zero(o.listed_op);
    out->listed_flag = data_or_zero(o.listed_flag);
    out->rflag = data_or_zero(o.rflag);
    out->spine_op = data_or_zero(o.spine_op);
    return HSC_OK;
}

int hsc_dep_graph_build_lists(hsc_ctx *c, int flags, hsc_graph_stats *st)
{
    if (!c) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    const ListBufs &l = c->lists;
    if (!l.valid) return ctx_fail(c, HSC_ESTATE, "no resolved list history (hsc_dep_graph_resolve_lists)");
    // the entry's rows take the staged pairs' slot: both cannot join one build
    if (c->graph.n_extra)
        return ctx_fail(c, HSC_EINVAL, "staged rw pairs cannot join a build from a list history");
    // no ops: graph_build finds no writers, emits no edges of its own and
    // sorts the rows of the x slot (holes dropped) like any staged rows
    GraphInput in{nullptr, nullptr, nullptr, nullptr, 0, l.nc};
    in.x_rows = l.x_rows.as<uint64_t>();
    in.x_type = l.x_type.as<uint64_t>();
    in.n_extra = l.n_rows;
    float build_ms = 0;
    const int rc = graph_build_timed(c, in, (flags & HSC_GRAPH_FULL) != 0, &build_ms);
    return build_stats(c, rc, build_ms, st);
}

// The internal-consistency pass over the history `in` names (the last
// successful resolve's, still on the device), timed; r: that resolve's sort
// rows.  Caller holds c->mu.
static int internal_timed(hsc_ctx *c, const InternalIn &in, ResolveBufs &r, unsigned flags, hsc_internal_report *out)
{
    hipStream_t s = c->stream;
    const bool arrays = (flags & HSC_INTERNAL_ARRAYS) != 0;
    EventSpan t;
    InternalOut &o = c->internal_out;
    hipError_t e = t.begin(s);
    if (e == hipSuccess) e = graph_internal(in, r, c->internal, arrays, o, s);
    if (e == hipSuccess) e = t.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    memset(out, 0, sizeof *out);
    HIPCHK(c, e);
    out->nops = o.nops;
    out->ntxn = o.ntxn;
    out->checked_reads = o.checked_reads;
    out->bad_reads = o.bad_reads;
    out->compared_elements = o.compared_elements;
    out->bad_txns = o.bad_txns;
    out->txn_bad = data_or_zero(o.txn_bad);
    out->n_listed = o.n_listed;
    out->listed_op = data_or_zero(o.listed_op);
    out->listed_anchor = data_or_zero(o.listed_anchor);
    out->bad = data_or_zero(o.bad);
    out->anchor_op = data_or_zero(o.anchor_op);
    out->sort_packed = o.sort_packed;
    out->ms = o.nops ? t.ms() : 0;
    return HSC_OK;
}

int hsc_dep_graph_internal(hsc_ctx *c, unsigned flags, hsc_internal_report *out)
{
    if (!c || !out) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    ResolveBufs &r = c->resolve;
    if (!r.valid) return ctx_fail(c, HSC_ESTATE, "no resolved history (hsc_dep_graph_resolve)");
    InternalIn in{};
    in.nops = r.in_nops;
    in.ntxn = r.in_ntxn;
    in.txn = r.in_txn.as<uint32_t>();
    in.key = r.in_key.as<uint64_t>();
    in.isw = r.in_isw.as<uint8_t>();
    in.value = r.in_val.as<uint64_t>();
    in.level = r.level.as<uint32_t>();
    return internal_timed(c, in, r, flags, out);
}

int hsc_dep_graph_internal_lists(hsc_ctx *c, unsigned flags, hsc_internal_report *out)
{
    if (!c || !out) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    ListBufs &l = c->lists;
    if (!l.valid) return ctx_fail(c, HSC_ESTATE, "no resolved list history (hsc_dep_graph_resolve_lists)");
    InternalIn in{};
    in.nops = l.in_nops;
    in.ntxn = l.in_ntxn;
    in.txn = l.in_txn.as<uint32_t>();
    in.key = l.in_key.as<uint64_t>();
    in.isw = l.in_isw.as<uint8_t>();
    in.value = l.in_val.as<uint64_t>();
    in.off = l.in_off.as<uint64_t>();
    in.elems = l.in_elems.as<uint64_t>();
    in.status = l.in_status.as<uint8_t>();
    in.lists = true;
    return internal_timed(c, in, l.t, flags, out);
}

int hsc_dep_graph_stage_rw_pairs(hsc_ctx *c, uint32_t nrs, const uint32_t *readset_txn,
                                 size_t ncommit, const uint64_t *commit_lsn,
                                 const uint32_t *commit_txn)
{
    if (!c || (nrs && !readset_txn) || (ncommit && (!commit_lsn || !commit_txn)))
        return HSC_EINVAL;
    GRAPH_ENTRY(c);
    for (size_t i = 1; i < ncommit; ++i)
        if (commit_lsn[i] <= commit_lsn[i - 1]) return ctx_fail(c, HSC_EINVAL, "commit LSNs not sorted");
    hipStream_t s = c->stream;
    GraphBufs &gb = c->graph;
    const size_t n = c->e_dev_n;
    gb.n_extra = 0;
    // every endpoint a pair can map to; graph_build_timed rejects the staged
    // rows if the build's ntxn does not cover them
    uint32_t xm = 0;
    for (uint32_t i = 0; i < nrs; ++i) xm = std::max(xm, readset_txn[i]);
    for (size_t i = 0; i < ncommit; ++i) xm = std::max(xm, commit_txn[i]);
    c->x_max_txn = xm;
    if (n == 0) return HSC_OK;
    // mapping tables next to each other: rs_txn[nrs] | commit_txn[ncommit] | commit_lsn[ncommit]
    const size_t o_ct = ((size_t)nrs + 1) & ~(size_t)1, o_cl = o_ct + ncommit + (ncommit & 1);
    HIPCHK(c, gb.x_map.ensure(4 * (o_cl + 2 * ncommit) + 64));
    uint32_t *m32 = gb.x_map.as<uint32_t>();
    uint64_t *cl = (uint64_t *)(m32 + o_cl);
    uint32_t *bad = m32 + o_cl + 2 * ncommit;
    if (nrs) HIPCHK(c, hipMemcpyAsync(m32, readset_txn, 4 * (size_t)nrs, hipMemcpyHostToDevice, s));
    if (ncommit) {
        HIPCHK(c, hipMemcpyAsync(m32 + o_ct, commit_txn, 4 * ncommit, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemcpyAsync(cl, commit_lsn, 8 * ncommit, hipMemcpyHostToDevice, s));
    }
    HIPCHK(c, hipMemsetAsync(bad, 0, 4, s));
    HIPCHK(c, gb.x_rows.ensure(8 * n));
    HIPCHK(c, gb.x_type.ensure(8 * n));
    HIPCHK(c, graph_pairs_rows(n, c->e_dev_txn, c->e_dev_lsn, nrs, m32, ncommit, cl, m32 + o_ct,
                               gb.x_rows.as<uint64_t>(), gb.x_type.as<uint64_t>(), bad, s));
    uint32_t hb = 0;
    HIPCHK(c, hipMemcpyAsync(&hb, bad, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (hb) return ctx_fail(c, HSC_EINVAL, "rw pair names a writer LSN or read set not in the map");
    gb.n_extra = n;
    return HSC_OK;
}

int hsc_dep_graph_stage_realtime(hsc_ctx *c, uint32_t ntxn, const uint64_t *invoke, const uint64_t *complete,
                                 uint64_t *n_edges, float *ms)
{
    if (!c || (ntxn && (!invoke || !complete))) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    GraphBufs &gb = c->graph;
    gb.rt_staged = false;  // a second call replaces the first; a failed one stages nothing
    gb.n_rt = 0;
    if (n_edges) *n_edges = 0;
    if (ms) *ms = 0;
    for (uint32_t v = 0; v < ntxn; ++v)
        if (invoke[v] > complete[v]) return ctx_fail(c, HSC_EINVAL, "a txn completes before its invoke");
    hipStream_t s = c->stream;
    EventSpan t;
    hipError_t e = t.begin(s);
    if (e == hipSuccess) e = realtime_stage(ntxn, invoke, complete, gb, s);
    if (e == hipErrorInvalidValue)
        return ctx_fail(c, HSC_EINVAL, "the real-time order has more edges than a build takes");
    if (e == hipSuccess) e = t.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) gb.n_rt = 0;
    HIPCHK(c, e);
    if (ms) *ms = t.ms();
    gb.rt_staged = true;
    if (n_edges) *n_edges = gb.n_rt;
    return HSC_OK;
}

int hsc_dep_graph_scc_built(hsc_ctx *c, uint32_t *scc_out, hsc_graph_stats *st)
{
    if (!c) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    const uint32_t nn = c->graph_ntxn;
    if (nn && !scc_out) return HSC_EINVAL;
    if (c->graph.raw) return ctx_fail(c, HSC_ESTATE, "last build kept raw rows only (no HSC_GRAPH_FULL)");
    return scc_timed(c, nn, scc_out, st);
}

int hsc_dep_graph_anomalies(hsc_ctx *c, unsigned flags, unsigned max_anti_batches, hsc_anomalies *out)
{
    if (!c || !out) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    GraphBufs &gb = c->graph;
    const uint32_t nn = c->graph_ntxn;
    if (gb.raw) return ctx_fail(c, HSC_ESTATE, "last build kept raw rows only (no HSC_GRAPH_FULL)");
    hipStream_t s = c->stream;
    EventSpan t;
    HIPCHK(c, t.begin(s));
    AnomOut &o = c->anom_out;
    hipError_t e = graph_anomalies(nn, gb, c->anom, (flags & HSC_ANOM_WITNESS) != 0, max_anti_batches, o, s);
    if (e == hipSuccess) e = t.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    memset(out, 0, sizeof *out);
    HIPCHK(c, e);
    out->ms = t.ms();
    out->ntxn = nn;
    out->cls = data_or_zero(o.cls);
    out->ncomp = (uint32_t)o.comp_label.size();
    out->comp_label = data_or_zero(o.comp_label);
    out->comp_class = data_or_zero(o.comp_class);
    if (o.wit_off.size() != (size_t)out->ncomp + 1) o.wit_off.assign((size_t)out->ncomp + 1, 0);
    out->wit_off = o.wit_off.data();
    out->wit_txn = data_or_zero(o.wit_txn);
    out->wit_type = data_or_zero(o.wit_type);
    for (int k = 0; k < 3; ++k) {
        out->comps[k] = o.comps[k];
        out->txns[k] = o.txns[k];
    }
    out->anti_edges = o.anti_edges;
    out->anti_tested = o.anti_tested;
    out->core_nodes = o.core_nodes;
    out->reach_batches = o.reach_batches;
    out->sweeps = (uint32_t)std::min<uint64_t>(o.sweeps, 0xFFFFFFFFull);
    out->bfs_levels = o.bfs_levels;
    return HSC_OK;
}

int hsc_dep_graph_si(hsc_ctx *c, unsigned flags, hsc_si_report *out)
{
    if (!c || !out) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    GraphBufs &gb = c->graph;
    const uint32_t nn = c->graph_ntxn;
    if (gb.raw) return ctx_fail(c, HSC_ESTATE, "last build kept raw rows only (no HSC_GRAPH_FULL)");
    hipStream_t s = c->stream;
    EventSpan t;
    HIPCHK(c, t.begin(s));
    SiOut &o = c->si_out;
    hipError_t e = graph_si(nn, gb, c->si, (flags & HSC_SI_WITNESS) != 0, o, s);
    const bool too_big = o.too_big;
    if (e == hipSuccess) e = t.end(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    memset(out, 0, sizeof *out);
    if (e != hipSuccess) {
        o.clear(0);
        out->nonadj = out->comp_nonadj = out->wit_type = (const uint8_t *)kZeros;
        out->comp_label = out->wit_off = out->wit_txn = (const uint32_t *)kZeros;
        if (too_big) return ctx_fail(c, HSC_EINVAL, "the product graph does not fit 32-bit node or edge ids");
    }
    HIPCHK(c, e);
    out->ms = t.ms();
    out->ntxn = nn;
    out->nonadj = data_or_zero(o.nonadj);
    out->ncomp = (uint32_t)o.comp_label.size();
    out->comp_label = data_or_zero(o.comp_label);
    out->comp_nonadj = data_or_zero(o.comp_nonadj);
    if (o.wit_off.size() != (size_t)out->ncomp + 1) o.wit_off.assign((size_t)out->ncomp + 1, 0);
    out->wit_off = o.wit_off.data();
    out->wit_txn = data_or_zero(o.wit_txn);
    out->wit_type = data_or_zero(o.wit_type);
    out->comps = o.comps;
    out->txns = o.txns;
    out->core_nodes = o.core_nodes;
    out->product_nodes = o.product_nodes;
    out->product_edges = o.product_edges;
    out->scc_rounds = o.scc_rounds;
    out->scc_iterations = o.scc_iterations;
    out->bfs_levels = o.bfs_levels;
    return HSC_OK;
}

int hsc_dep_graph_cover(hsc_ctx *c, uint8_t *cover_dev)
{
    if (!c || (c->graph_ntxn && !cover_dev)) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    HIPCHK(c, graph_cover(c->graph, c->graph_ntxn, cover_dev, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HSC_OK;
}

int hsc_dep_graph_cut(hsc_ctx *c, const uint8_t *cover_dev, uint64_t *rows_dev, size_t cap,
                      size_t *m)
{
    if (!c || !m || (c->graph_ntxn && !cover_dev)) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    HIPCHK(c, graph_cut(c->graph, cover_dev, m, c->stream));
    const size_t k = std::min(cap, *m);
    if (k && rows_dev)
        HIPCHK(c, hipMemcpyAsync(rows_dev, c->graph.cut.p, 8 * k, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HSC_OK;
}

int hsc_dep_graph_scc_cut(hsc_ctx *c, uint32_t ntxn, const uint8_t *cover_dev,
                          const uint64_t *rows_dev, size_t m, uint32_t *scc_dev,
                          hsc_graph_stats *st)
{
    if (!c || (ntxn && (!cover_dev || !scc_dev)) || (m && !rows_dev) || m > 0xFFFFFFFFull)
        return HSC_EINVAL;
    GRAPH_ENTRY(c);
    hipStream_t s = c->stream;
    EventSpan t;
    HIPCHK(c, t.begin(s));
    uint32_t rounds = 0, iters = 0, nc = 0;
    hipError_t e = graph_scc_rows(ntxn, cover_dev, rows_dev, m, c->subgraph, scc_dev, &nc, &rounds,
                                  &iters, s);
    if (e == hipErrorInvalidValue) return ctx_fail(c, HSC_EINVAL, "cut row outside the cover");
    HIPCHK(c, e);
    HIPCHK(c, t.end(s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (!st) return HSC_OK;
    memset(st, 0, sizeof *st);
    st->edges = c->subgraph.ne;
    st->scc_ms = t.ms();
    st->rounds = rounds;
    st->iterations = iters;
    st->cut_nodes = nc;
    // components of >= 2 txns live in the cut: its nc colours suffice
    std::vector<uint32_t> h(std::max<uint32_t>(nc, 1));
    if (nc) HIPCHK(c, hipMemcpy(h.data(), c->subgraph.scc.p, 4 * (size_t)nc, hipMemcpyDeviceToHost));
    scc_size_stats(h.data(), nc, st);
    return HSC_OK;
}

int hsc_dep_graph_edges(hsc_ctx *c, uint32_t *src, uint32_t *dst, uint32_t *type, size_t cap,
                        size_t *n)
{
    if (!c || !n) return HSC_EINVAL;
    GRAPH_ENTRY(c);
    GraphBufs &gb = c->graph;
    *n = gb.ne;
    const size_t m = std::min(cap, gb.ne);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (m && src) HIPCHK(c, hipMemcpy(src, gb.src.p, 4 * m, hipMemcpyDeviceToHost));
    if (m && dst) HIPCHK(c, hipMemcpy(dst, gb.out_dst.p, 4 * m, hipMemcpyDeviceToHost));
    if (m && type) HIPCHK(c, hipMemcpy(type, gb.type.p, 4 * m, hipMemcpyDeviceToHost));
    return HSC_OK;
}

}  // extern "C"

// The cut of the last build under cover (one pass: count + rows); *rows
// points into the context's own buffer until its next graph call.
int hsc::ctx_graph_cut(hsc_ctx *c, const uint8_t *cover, size_t *m, const uint64_t **rows, const uint32_t *op_txn,
                       const uint64_t *op_key, const uint8_t *op_isw)
{
    MuGuard g(c);
    (void)hipSetDevice(c->device);
    HIPCHK(c, graph_cut(c->graph, cover, m, c->stream, op_txn, op_key, op_isw, false));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *rows = c->graph.cut.as<uint64_t>();
    return HSC_OK;
}
