// hsc_si.hip -- snapshot isolation from the dependency graph: which cycles have
// no two adjacent anti-dependency edges, and one witness cycle per violating
// component, on gfx950.
//
// Input: as hsc_anomaly.hip -- the typed edges of the last full build and
// graph_scc's labels.  E1 = the edges carrying a ww, wr or rt bit; an anti
// edge has type == 4 exactly.  Snapshot isolation allows a dependency graph
// iff every cycle has two adjacent anti edges (Cerone and Gotsman; Elle's
// G-nonadjacent), so it is violated iff some cycle has no two cyclically
// consecutive anti edges.
//
// Product graph P over the core (the txns of components of >= 2 txns): core
// node u becomes 2u ("reached by an E1 edge") and 2u + 1 ("reached by an anti
// edge").  An E1 edge u -> v gives 2u -> 2v and 2u + 1 -> 2v; an anti edge
// gives 2u -> 2v + 1 only -- no anti edge leaves a node an anti edge reached.
// A closed walk of P projects to a closed walk of the core without two
// cyclically consecutive anti edges, and every such walk lifts to P by the
// type of each arriving edge.  nonadj[u] = 2u or 2u + 1 lies in a component of
// P with >= 2 nodes.
//
// Steps:
//   core     graph_core (hsc_anomaly.hip) into buffers of this analysis
//   CSR      P's row starts are closed form in the core's typed CSR offsets
//            coff and the E1 offsets off1: row 2u starts at coff[u] + off1[u]
//            and holds every out-edge of u, row 2u + 1 starts at coff[u + 1] +
//            off1[u] and holds the E1 ones.  A thread per core edge stores its
//            one or two lifts; rows stay in (src, dst) order.
//   CSC      in-degrees by atomics in the same pass (2 per E1 edge at 2v, 1
//            per anti edge at 2v + 1), an exclusive scan, a fill through a
//            cursor per node
//   SCC      graph_scc over the 2 nc nodes, in a GraphBufs of its own
//   fold     the members of P's components of >= 2 nodes, OR-ed per core node;
//            a component of the build is flagged when a member has the bit
//   witness  per flagged component the lowest core edge a lift a' -> b' of
//            which stays inside a component of P, then one level-synchronous
//            BFS over P from every b' at once, restricted to b''s component of
//            P, parents claimed with atomicCAS, until every a' is reached.  The
//            host walks the parents back, projects the walk to txns and cuts
//            it down to a simple cycle.
#include "hsc_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace hsc {

namespace {
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kSelf = 0xFFFFFFFEu;  // parent slot of a BFS source
constexpr uint32_t kE1 = (uint32_t)(kDepWW | kDepWR | kDepRT);
constexpr uint32_t kAnti = (uint32_t)kDepRW;
inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

// poff[2u] = coff[u] + off1[u], poff[2u + 1] = coff[u + 1] + off1[u], u in [0, nc];
// poff[2 nc] = me + m1
__global__ void k_si_offsets(uint32_t nc, const uint32_t *coff, const uint32_t *off1, uint32_t *poff)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u > nc) return;
    const uint32_t c = coff[u], o = off1[u];
    poff[2 * (size_t)u] = c + o;
    if (u < nc) poff[2 * (size_t)u + 1] = coff[u + 1] + o;
}

// Core edge e = u -> v: its lift from 2u in row 2u at e's place among u's
// edges, an E1 edge's second lift from 2u + 1 at its place among u's E1 edges
// (p1 = the exclusive scan of the E1 flags).  indeg: P's in-degrees.
__global__ void k_si_emit(uint32_t me, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *ctype,
                          const uint32_t *coff, const uint32_t *off1, const uint32_t *p1,
                          const uint32_t *poff, uint32_t *pdst, uint32_t *indeg)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= me) return;
    const uint32_t u = csrc[e], v = cdst[e], t = ctype[e];
    if (t & kE1) {
        pdst[poff[2 * (size_t)u] + (e - coff[u])] = 2 * v;
        pdst[poff[2 * (size_t)u + 1] + (p1[e] - off1[u])] = 2 * v;
        atomicAdd(&indeg[2 * (size_t)v], 2u);
    } else {
        pdst[poff[2 * (size_t)u] + (e - coff[u])] = 2 * v + 1;
        atomicAdd(&indeg[2 * (size_t)v + 1], 1u);
    }
}

// in-rows by a cursor per node (their order inside a node's rows is free)
__global__ void k_si_infill(uint32_t me, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *ctype,
                            uint32_t *cursor, uint32_t *in_src)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= me) return;
    const uint32_t u = csrc[e], v = cdst[e];
    if (ctype[e] & kE1) {
        const uint32_t at = atomicAdd(&cursor[2 * (size_t)v], 2u);
        in_src[at] = 2 * u;
        in_src[at + 1] = 2 * u + 1;
    } else {
        in_src[atomicAdd(&cursor[2 * (size_t)v + 1], 1u)] = 2 * u;
    }
}

// nonadj[u] = either state of u is a member; a flagged node flags its component
// (plain stores of 1: every writer writes the same value)
__global__ void k_si_fold(uint32_t nc, const uint32_t *pm, const uint32_t *comp_of, uint32_t *nonadj,
                          uint32_t *cflag)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nc) return;
    const uint32_t b = (pm[2 * (size_t)u] | pm[2 * (size_t)u + 1]) != 0;
    nonadj[u] = b;
    if (b) cflag[comp_of[u]] = 1;
}

// wmin[c]: the lowest core edge of component c with a lift inside a component of P
__global__ void k_si_wmin(uint32_t me, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *ctype,
                          const uint32_t *pscc, const uint32_t *comp_of, uint32_t *wmin)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= me) return;
    const uint32_t u = csrc[e], v = cdst[e];
    bool in;
    if (ctype[e] & kE1) {
        const uint32_t lv = pscc[2 * (size_t)v];
        in = pscc[2 * (size_t)u] == lv || pscc[2 * (size_t)u + 1] == lv;
    } else {
        in = pscc[2 * (size_t)u] == pscc[2 * (size_t)v + 1];
    }
    if (in) atomicMin(&wmin[comp_of[u]], e);
}

__global__ void k_si_bfs_init(uint32_t nw, const uint32_t *wsrc, const uint32_t *wtgt, uint32_t *par,
                              uint32_t *target, uint32_t *front)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nw) return;
    par[wsrc[c]] = kSelf;
    target[wtgt[c]] = 1;
    front[c] = wsrc[c];
}

// One BFS level over P inside the sources' components of P; par[w] = the node
// that claimed w.  cnt[0]: the next frontier's size; cnt[1]: targets reached
__global__ void k_si_bfs_step(const uint32_t *front, uint32_t nf, const uint32_t *poff, const uint32_t *pdst,
                              const uint32_t *pscc, uint32_t *par, const uint32_t *target, uint32_t *next,
                              uint32_t *cnt)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nf) return;
    const uint32_t x = front[k], lx = pscc[x];
    for (uint32_t e = poff[x]; e < poff[x + 1]; ++e) {
        const uint32_t w = pdst[e];
        if (pscc[w] != lx) continue;
        if (__hip_atomic_load(&par[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kNone) continue;
        if (atomicCAS(&par[w], kNone, x) != kNone) continue;
        next[atomicAdd(&cnt[0], 1u)] = w;
        if (target[w]) atomicAdd(&cnt[1], 1u);
    }
}

void SiBufs::release_all()
{
    DBuf *all[] = {&pm, &nonadj, &cflag, &wmin, &wsrc, &wtgt, &par, &target, &front, &front2, &cnt};
    for (DBuf *b : all) b->release();
    core.release_core();
    p.release_all();
}

namespace {
struct Step {
    uint32_t txn;
    uint8_t type;  // of the edge to the next step (cyclically)
};

// A closed walk without two cyclically consecutive anti edges -> a simple
// cycle with the same property: split at the first repeated txn into the two
// closed halves.  A half inherits every adjacency but the one at the split; if
// that one joins two anti edges in one half, both edges of the other half
// there are not anti edges.  Keep a good half, the shorter if both are.
bool reduce_walk(std::vector<Step> &w, std::vector<uint32_t> &seen_at, std::vector<Step> &tmp)
{
    for (;;) {
        const size_t L = w.size();
        size_t i = L, j = L;
        for (size_t k = 0; k < L; ++k) {
            uint32_t &at = seen_at[w[k].txn];
            if (at != kNone) {
                i = at;
                j = k;
                break;
            }
            at = (uint32_t)k;
        }
        for (size_t k = 0; k < L && k <= j; ++k) seen_at[w[k].txn] = kNone;
        if (j == L) return true;
        // inner: steps [i, j); outer: steps [0, i) + [j, L)
        const bool in_ok = !(w[j - 1].type == kAnti && w[i].type == kAnti);
        const bool out_ok = !(w[(i + L - 1) % L].type == kAnti && w[j].type == kAnti);
        if (!in_ok && !out_ok) return false;
        const bool inner = in_ok && (!out_ok || j - i <= L - (j - i));
        tmp.clear();
        if (inner) {
            tmp.assign(w.begin() + i, w.begin() + j);
        } else {
            tmp.assign(w.begin(), w.begin() + i);
            tmp.insert(tmp.end(), w.begin() + j, w.end());
        }
        if (tmp.size() < 2) return false;
        w.swap(tmp);
    }
}
}  // namespace

hipError_t graph_si(uint32_t nn, GraphBufs &g, SiBufs &si, bool witness, SiOut &out, hipStream_t s)
{
    hipError_t e = hipSuccess;
#define CK(x)                                 \
    do {                                      \
        e = (x);                              \
        if (e != hipSuccess) return e;        \
    } while (0)
    out.clear(nn);
    if (nn == 0) return hipSuccess;
    CoreBufs &a = si.core;
    CoreDims cd;
    CK(graph_core(nn, g, a, cd, &out.scc_rounds, &out.scc_iterations, s));
    const uint32_t nc = cd.nc, ncomp = cd.ncomp, me = cd.me, m1 = cd.m1;
    out.core_nodes = nc;
    if (nc == 0) return hipSuccess;
    if (cd.na != me - m1) return hipErrorUnknown;  // an edge is E1 or an anti edge
    if (nc > 0x7FFFFFFEu || (uint64_t)me + m1 > 0xFFFFFFFEull) {
        out.too_big = true;
        return hipErrorInvalidValue;
    }
    const uint32_t np = 2 * nc, mp = me + m1;
    out.product_nodes = np;
    out.product_edges = mp;

    // ---- b / c. P's CSR and CSC ----
    GraphBufs &p = si.p;
    CK(p.out_off.ensure(4 * ((size_t)np + 1)));
    CK(p.in_off.ensure(4 * ((size_t)np + 1)));
    CK(p.flags.ensure(4 * ((size_t)np + 1)));  // the CSC fill's cursors
    CK(p.out_dst.ensure(4 * ((size_t)mp + 1)));
    CK(p.in_src.ensure(4 * ((size_t)mp + 1)));
    const uint32_t *coff = a.coff.as<uint32_t>(), *off1 = a.e1.out_off.as<uint32_t>();
    const uint32_t *csrc = a.csrc.as<uint32_t>(), *cdst = a.cdst.as<uint32_t>(), *ctype = a.ctype.as<uint32_t>();
    k_si_offsets<<<blocks((size_t)nc + 1), 256, 0, s>>>(nc, coff, off1, p.out_off.as<uint32_t>());
    CK(hipMemsetAsync(p.in_off.p, 0, 4 * ((size_t)np + 1), s));
    k_si_emit<<<blocks(me), 256, 0, s>>>(me, csrc, cdst, ctype, coff, off1, a.f1.as<uint32_t>(),
                                         p.out_off.as<uint32_t>(), p.out_dst.as<uint32_t>(),
                                         p.in_off.as<uint32_t>());
    CK(a.scratch.ensure(scan_scratch_bytes((size_t)np + 1) + 64));
    CK(scan_exclusive_u32(p.in_off.as<uint32_t>(), (size_t)np + 1, a.scratch.as<uint32_t>(), s));
    CK(hipMemcpyAsync(p.flags.p, p.in_off.p, 4 * ((size_t)np + 1), hipMemcpyDeviceToDevice, s));
    k_si_infill<<<blocks(me), 256, 0, s>>>(me, csrc, cdst, ctype, p.flags.as<uint32_t>(), p.in_src.as<uint32_t>());
    CK(hipGetLastError());

    // ---- d. the components of P ----
    uint32_t rp = 0, ip = 0;
    // (the colouring appends a node to its frontier once per colour it takes
    // in a step: room for a push per row on top of graph_scc's own sizing)
    CK(p.front.ensure(4 * ((size_t)np + mp) + 64));
    CK(p.front2.ensure(4 * ((size_t)np + mp) + 64));
    CK(graph_scc(np, p, &rp, &ip, s));
    out.scc_rounds += rp;
    out.scc_iterations += ip;
    const uint32_t *pscc = p.scc.as<uint32_t>();

    // ---- e. fold ----
    CK(si.pm.ensure(4 * (size_t)np));
    CK(si.nonadj.ensure(4 * (size_t)nc));
    CK(si.cflag.ensure(4 * (size_t)ncomp));
    CK(hipMemsetAsync(si.pm.p, 0, 4 * (size_t)np, s));
    CK(hipMemsetAsync(si.cflag.p, 0, 4 * (size_t)ncomp, s));
    CK(scc_members(np, pscc, si.pm.as<uint32_t>(), s));
    k_si_fold<<<blocks(nc), 256, 0, s>>>(nc, si.pm.as<uint32_t>(), a.comp_of.as<uint32_t>(),
                                         si.nonadj.as<uint32_t>(), si.cflag.as<uint32_t>());
    CK(hipGetLastError());

    // ---- results: per txn, per component ----
    std::vector<uint32_t> node_txn(nc), bit(nc), cflag(ncomp);
    out.comp_label.resize(ncomp);
    CK(hipMemcpyAsync(node_txn.data(), a.node_txn.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(bit.data(), si.nonadj.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(cflag.data(), si.cflag.p, 4 * (size_t)ncomp, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(out.comp_label.data(), a.comp_label.p, 4 * (size_t)ncomp, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    for (uint32_t u = 0; u < nc; ++u) {
        if (node_txn[u] >= nn) return hipErrorUnknown;
        out.nonadj[node_txn[u]] = (uint8_t)(bit[u] != 0);
        out.txns += bit[u] != 0;
    }
    out.comp_nonadj.resize(ncomp);
    uint32_t nw = 0;
    for (uint32_t c = 0; c < ncomp; ++c) {
        out.comp_nonadj[c] = (uint8_t)(cflag[c] != 0);
        nw += cflag[c] != 0;
    }
    out.comps = nw;
    out.wit_off.assign((size_t)ncomp + 1, 0);
    if (!witness || nw == 0) return hipSuccess;

    // ---- f. witnesses ----
    CK(si.wmin.ensure(4 * (size_t)ncomp));
    CK(hipMemsetAsync(si.wmin.p, 0xFF, 4 * (size_t)ncomp, s));
    k_si_wmin<<<blocks(me), 256, 0, s>>>(me, csrc, cdst, ctype, pscc, a.comp_of.as<uint32_t>(),
                                         si.wmin.as<uint32_t>());
    std::vector<uint32_t> wmin(ncomp), hsrc(me), hdst(me), htype(me), hoff((size_t)nc + 1), hscc(np);
    CK(hipMemcpyAsync(wmin.data(), si.wmin.p, 4 * (size_t)ncomp, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(hsrc.data(), csrc, 4 * (size_t)me, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(hdst.data(), cdst, 4 * (size_t)me, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(htype.data(), ctype, 4 * (size_t)me, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(hoff.data(), coff, 4 * ((size_t)nc + 1), hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(hscc.data(), pscc, 4 * (size_t)np, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    // the closing lift a' -> b' of every flagged component, state 0 of a first
    std::vector<uint32_t> wc, close, wsrc, wtgt;
    for (uint32_t c = 0; c < ncomp; ++c) {
        if (!cflag[c]) continue;
        const uint32_t ce = wmin[c];
        if (ce >= me) return hipErrorUnknown;  // a component of P with >= 2 nodes holds an edge
        const uint32_t u = hsrc[ce], v = hdst[ce];
        if (u >= nc || v >= nc) return hipErrorUnknown;
        const bool anti = !(htype[ce] & kE1);
        const uint32_t b = 2 * v + (anti ? 1u : 0u);
        uint32_t ap = 2 * u;
        if (hscc[ap] != hscc[b]) {
            ap = 2 * u + 1;
            if (anti || hscc[ap] != hscc[b]) return hipErrorUnknown;
        }
        wc.push_back(c);
        close.push_back(ce);
        wsrc.push_back(b);
        wtgt.push_back(ap);
    }
    CK(si.wsrc.ensure(4 * (size_t)nw));
    CK(si.wtgt.ensure(4 * (size_t)nw));
    CK(si.par.ensure(4 * (size_t)np));
    CK(si.target.ensure(4 * (size_t)np));
    CK(si.front.ensure(4 * (size_t)np + 64));
    CK(si.front2.ensure(4 * (size_t)np + 64));
    CK(si.cnt.ensure(64));
    CK(hipMemcpyAsync(si.wsrc.p, wsrc.data(), 4 * (size_t)nw, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(si.wtgt.p, wtgt.data(), 4 * (size_t)nw, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(si.par.p, 0xFF, 4 * (size_t)np, s));
    CK(hipMemsetAsync(si.target.p, 0, 4 * (size_t)np, s));
    uint32_t *cnt = si.cnt.as<uint32_t>();
    CK(hipMemsetAsync(cnt, 0, 8, s));
    k_si_bfs_init<<<blocks(nw), 256, 0, s>>>(nw, si.wsrc.as<uint32_t>(), si.wtgt.as<uint32_t>(),
                                             si.par.as<uint32_t>(), si.target.as<uint32_t>(),
                                             si.front.as<uint32_t>());
    uint32_t *f = si.front.as<uint32_t>(), *f2 = si.front2.as<uint32_t>();
    uint32_t nf = nw, found = 0;
    while (nf && found < nw) {
        ++out.bfs_levels;
        uint32_t h[2] = {0, 0};
        CK(hipMemsetAsync(cnt, 0, 4, s));
        k_si_bfs_step<<<blocks(nf), 256, 0, s>>>(f, nf, p.out_off.as<uint32_t>(), p.out_dst.as<uint32_t>(), pscc,
                                                 si.par.as<uint32_t>(), si.target.as<uint32_t>(), f2, cnt);
        CK(hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        nf = h[0];
        found = h[1];
        if (nf > np) return hipErrorUnknown;  // every node is claimed once
        std::swap(f, f2);
    }
    if (found < nw) return hipErrorUnknown;  // a' and b' share a component of P
    std::vector<uint32_t> par(np);
    CK(hipMemcpyAsync(par.data(), si.par.p, 4 * (size_t)np, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    // type bits of the core edge x -> y (rows sorted by dst)
    auto edge_type = [&](uint32_t x, uint32_t y, uint32_t &t) {
        const uint32_t *lo = hdst.data() + hoff[x], *hi = hdst.data() + hoff[x + 1];
        const uint32_t *it = std::lower_bound(lo, hi, y);
        if (it == hi || *it != y) return false;
        t = htype[it - hdst.data()];
        return true;
    };
    std::vector<uint32_t> rev, seen_at(nn, kNone);
    std::vector<Step> walk, tmp;
    size_t k = 0;
    for (uint32_t c = 0; c < ncomp; ++c) {
        if (k < nw && wc[k] == c) {
            rev.clear();
            for (uint32_t w = wtgt[k]; w != wsrc[k];) {  // P nodes from a' back to b'
                if (w >= np || rev.size() > np) return hipErrorUnknown;
                rev.push_back(w);
                w = par[w];
            }
            // the walk b, ..., a: a step's type is that of the edge to the next
            // node, the arriving edge of that node's state
            walk.clear();
            uint32_t at = wsrc[k];
            for (size_t q = rev.size(); q-- > 0;) {
                const uint32_t nx = rev[q];
                uint32_t t = 0;
                if (!edge_type(at >> 1, nx >> 1, t)) return hipErrorUnknown;
                if (((nx & 1) != 0) != (t == kAnti)) return hipErrorUnknown;
                walk.push_back(Step{node_txn[at >> 1], (uint8_t)t});
                at = nx;
            }
            walk.push_back(Step{node_txn[at >> 1], (uint8_t)htype[close[k]]});
            if (!reduce_walk(walk, seen_at, tmp)) return hipErrorUnknown;
            for (const Step &st : walk) {
                out.wit_txn.push_back(st.txn);
                out.wit_type.push_back(st.type);
            }
            ++k;
        }
        out.wit_off[c + 1] = (uint32_t)out.wit_txn.size();
    }
#undef CK
    return hipSuccess;
}

// load this file's code object now (see warm_graph)
hipError_t warm_si()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_si_emit);
}

}  // namespace hsc
