// hsc_anomaly.hip -- which anomaly a dependency cycle is (G1c / G-single / G2)
// and one witness cycle per component, on gfx950.
//
// Input: the typed edges of the last full build (GraphBufs src / out_dst /
// type sorted by (src, dst), type bits 1 ww, 2 wr, 4 rw, 8 rt -- the real-time
// order of hsc_realtime.hip, present only when it was staged) and graph_scc's
// labels.  E1 = the edges carrying a ww, wr or rt bit (type & kE1); an anti
// edge has type == 4 exactly, so an rw edge the real-time order also forces
// (rw | rt) is E1.  Without rt edges E1 is what it was; with them the three
// bits below keep their definitions over the widened E1.  Per txn: bit 1 (G1c) its component of (V, E1) has >= 2 txns; bit 2
// (G-single) an anti edge a -> b of its component closes a cycle b ~> v ~> a
// over E1 edges of the component; bit 4 (G2) its component holds an anti edge.
//
// Steps:
//   core     (graph_core, which hsc_si.hip calls as well) the txns of
//            nontrivial components relabelled densely (txn order) and the
//            edges inside a component: a flag + scan compaction over the nodes
//            and over the edges; everything after it costs O(core)
//   G1c      graph_scc of the core restricted to E1 (its own GraphBufs; the
//            CSC by counting, the colouring does not need sorted rows)
//   G-single bit-parallel reach: the core's anti edges in (src, dst) order, 64
//            to a batch; per batch and node F (bit j: b_j reaches the node) and
//            B (bit j: the node reaches a_j), seeded at b_j / a_j and swept
//            over the E1 rows until a sweep changes nothing -- B pulled from
//            the out-neighbours, F pushed to them with a 64-bit atomic OR.
//            Up to 64 batches share a launch and the sweep's round trip, their
//            masks side by side per node.  A node with F & B != 0 lies on a
//            cycle with one anti edge; anti edge j is closed when F[a_j] has
//            bit j.
//   G2       a flag per component from one pass over the anti edges
//   witness  per component the lowest qualifying edge a -> b of its class, then
//            one level-synchronous BFS from every b at once (the core's edges
//            never leave a component), parent edges claimed with atomicCAS,
//            until every a is reached; the walk back runs on the host over the
//            core-sized arrays.
#include "hsc_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace hsc {

namespace {
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kSelf = 0xFFFFFFFEu;  // parent slot of a BFS source
// F and B of the batches one launch sweeps together: 64 batches up to 256 K core nodes
constexpr size_t kReachBytes = 256u << 20;
constexpr int kSweepsPerSync = 4;
constexpr uint32_t kE1 = (uint32_t)(kDepWW | kDepWR | kDepRT);
constexpr uint32_t kAnti = (uint32_t)kDepRW;
inline unsigned blocks(size_t n) { return (unsigned)((n + 255) / 256); }
}  // namespace

// flag[v] = flag[label[v]] = 1 for every v that is not its component's label:
// exactly the members of components of >= 2 nodes (flag zeroed by the caller)
__global__ void k_an_member(uint32_t n, const uint32_t *label, uint32_t *flag)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const uint32_t r = label[v];
    if (r != v && r < n) {
        flag[v] = 1;
        flag[r] = 1;
    }
}

// core node u = id[v] of member v; root[u]: v is its component's label
__global__ void k_an_nodes(uint32_t nn, const uint32_t *flag, const uint32_t *id, const uint32_t *scc,
                           uint32_t *node_txn, uint32_t *root)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nn || !flag[v]) return;
    const uint32_t u = id[v];
    node_txn[u] = v;
    root[u] = scc[v] == v;
}

// components in label order: cid = the exclusive scan of root[]
__global__ void k_an_comps(uint32_t nc, const uint32_t *node_txn, const uint32_t *scc, const uint32_t *id,
                           const uint32_t *cid, uint32_t *comp_of, uint32_t *comp_label)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nc) return;
    const uint32_t v = node_txn[u], r = scc[v];
    const uint32_t c = cid[id[r]];
    comp_of[u] = c;
    if (r == v) comp_label[c] = v;
}

__global__ void k_an_eflags(size_t ne, const uint32_t *src, const uint32_t *dst, const uint32_t *scc,
                            uint32_t *flags)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const uint32_t a = src[i], b = dst[i];
    flags[i] = a != b && scc[a] == scc[b];
}

__global__ void k_an_erows(size_t ne, const uint32_t *src, const uint32_t *dst, const uint32_t *type,
                           const uint32_t *scc, const uint32_t *pos, const uint32_t *id, uint32_t *csrc,
                           uint32_t *cdst, uint32_t *ctype)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ne) return;
    const uint32_t a = src[i], b = dst[i];
    if (a == b || scc[a] != scc[b]) return;
    const uint32_t p = pos[i];
    csrc[p] = id[a];
    cdst[p] = id[b];
    ctype[p] = type[i];
}

// the core's edges split: f1[i] E1, fa[i] anti
__global__ void k_an_split_flags(uint32_t me, const uint32_t *ctype, uint32_t *f1, uint32_t *fa)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= me) return;
    const uint32_t t = ctype[i];
    f1[i] = (t & kE1) != 0;
    fa[i] = t == kAnti;
}

// p1 / pa: the scans of f1 / fa.  E1 rows (src, dst, core edge) and the anti
// edges (a, b, core edge), both still in (src, dst) order
__global__ void k_an_split_rows(uint32_t me, const uint32_t *csrc, const uint32_t *cdst, const uint32_t *ctype,
                                const uint32_t *p1, const uint32_t *pa, uint32_t *s1, uint32_t *d1,
                                uint32_t *e1, uint32_t *aa, uint32_t *ab, uint32_t *ae)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= me) return;
    const uint32_t t = ctype[i];
    if (t & kE1) {
        const uint32_t p = p1[i];
        s1[p] = csrc[i];
        d1[p] = cdst[i];
        e1[p] = i;
    } else if (t == kAnti) {
        const uint32_t p = pa[i];
        aa[p] = csrc[i];
        ab[p] = cdst[i];
        ae[p] = i;
    }
}

// off[u] = first row whose key (sorted) is >= u, u in [0, n]
__global__ void k_an_offsets(uint32_t n, uint32_t m, const uint32_t *key, uint32_t *off)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u > n) return;
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key[mid] < u)
            lo = mid + 1;
        else
            hi = mid;
    }
    off[u] = lo;
}

__global__ void k_an_indeg(uint32_t m, const uint32_t *dst, uint32_t *deg)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) atomicAdd(&deg[dst[i]], 1u);
}

// in-rows by a cursor per node (their order inside a node's rows is free)
__global__ void k_an_infill(uint32_t m, const uint32_t *src, const uint32_t *dst, uint32_t *cursor,
                            uint32_t *in_src)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < m) in_src[atomicAdd(&cursor[dst[i]], 1u)] = src[i];
}

__global__ void k_an_g2(uint32_t na, const uint32_t *aa, const uint32_t *comp_of, uint32_t *cg2)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < na) cg2[comp_of[aa[j]]] = 1;
}

// ---- G-single: bit-parallel multi-source reach --------------------------------
// A launch sweeps G = 2^lg batches together; the masks lie node-major, F[u G +
// y] for batch y, and thread u G + y takes node u's batch y: the lanes of a
// wave share their node (G = 64) or a few nodes, so the row walk is uniform
// and every neighbour's masks are one contiguous read for the wave.
// anti edges [j0, j0 + n) of the group: bit (j - j0) % 64 of batch (j - j0) / 64
__global__ void k_an_reach_seed(uint32_t j0, uint32_t n, int lg, const uint32_t *aa, const uint32_t *ab,
                                unsigned long long *F, unsigned long long *B)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const unsigned long long bit = 1ull << (k & 63);
    atomicOr(&F[((size_t)ab[j0 + k] << lg) + (k >> 6)], bit);
    atomicOr(&B[((size_t)aa[j0 + k] << lg) + (k >> 6)], bit);
}

// One sweep over the E1 rows: node u pulls B from its out-neighbours and
// pushes F to them.  Values another workgroup wrote during this launch may or
// may not be seen -- the masks only grow, and a sweep in which nothing was
// written read the true masks, so it is the fixpoint.  *changed: one atomic
// per wave that changed something.
__global__ __launch_bounds__(256) void k_an_reach_sweep(size_t total, int lg, const uint32_t *off,
                                                        const uint32_t *dst, unsigned long long *F,
                                                        unsigned long long *B, uint32_t *changed)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool ch = false;
    if (i < total) {
        const uint32_t u = (uint32_t)(i >> lg);
        const size_t y = i & (((size_t)1 << lg) - 1);
        const unsigned long long fu = __hip_atomic_load(&F[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long bu = __hip_atomic_load(&B[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned long long nb = bu;
        for (uint32_t e = off[u]; e < off[u + 1]; ++e) {
            const size_t w = ((size_t)dst[e] << lg) + y;
            nb |= __hip_atomic_load(&B[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (fu & ~__hip_atomic_load(&F[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                ch |= (fu & ~atomicOr(&F[w], fu)) != 0;
        }
        if (nb != bu) {  // B[i] has this one writer
            __hip_atomic_store(&B[i], nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ch = true;
        }
    }
    const uint64_t m = __ballot(ch);
    if (m && (threadIdx.x & 63) == __ffsll((unsigned long long)m) - 1) atomicOr(changed, 1u);
}

// closed[j] = b_j reaches a_j
__global__ void k_an_reach_closed(uint32_t j0, uint32_t n, int lg, const uint32_t *aa,
                                  const unsigned long long *F, uint32_t *closed)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    closed[j0 + k] = (uint32_t)((F[((size_t)aa[j0 + k] << lg) + (k >> 6)] >> (k & 63)) & 1);
}

// F & B bit j: b_j ~> u ~> a_j, so a_j -> b_j closes a cycle through u
__global__ void k_an_reach_mark(size_t total, int lg, const unsigned long long *F, const unsigned long long *B,
                                uint32_t *gs)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total && (F[i] & B[i])) gs[i >> lg] = 1;
}

__global__ void k_an_cls(uint32_t nc, const uint32_t *g1c, const uint32_t *gs, const uint32_t *cg2,
                         const uint32_t *comp_of, uint32_t *cls)
{
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nc) return;
    cls[u] = (g1c[u] ? 1u : 0u) | (gs[u] ? 2u : 0u) | (cg2[comp_of[u]] ? 4u : 0u);
}

// ---- witnesses --------------------------------------------------------------------
// wmin[3 c + k]: the lowest core edge of component c that can close a cycle
// of class k (0 G1c: an E1 edge inside an E1 component; 1 G-single: a closed
// anti edge; 2 G2: an anti edge)
__global__ void k_an_wmin_e1(uint32_t m1, const uint32_t *s1, const uint32_t *d1, const uint32_t *e1,
                             const uint32_t *scc1, const uint32_t *comp_of, uint32_t *wmin)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m1) return;
    const uint32_t a = s1[i];
    if (scc1[a] == scc1[d1[i]]) atomicMin(&wmin[3 * comp_of[a]], e1[i]);
}

__global__ void k_an_wmin_anti(uint32_t na, const uint32_t *aa, const uint32_t *ae, const uint32_t *closed,
                               const uint32_t *comp_of, uint32_t *wmin)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= na) return;
    const uint32_t c = comp_of[aa[j]];
    atomicMin(&wmin[3 * c + 2], ae[j]);
    if (closed[j]) atomicMin(&wmin[3 * c + 1], ae[j]);
}

__global__ void k_an_bfs_init(uint32_t ncomp, const uint32_t *wsrc, const uint32_t *wtgt, uint32_t *pedge,
                              uint32_t *target, uint32_t *front)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncomp) return;
    pedge[wsrc[c]] = kSelf;
    target[wtgt[c]] = 1;
    front[c] = wsrc[c];
}

// cnt[0]: the next frontier's size; cnt[1]: targets reached so far
__global__ void k_an_bfs_step(const uint32_t *front, uint32_t nf, const uint32_t *off, const uint32_t *dst,
                              const uint32_t *type, const uint32_t *comp_of, const uint32_t *wmask,
                              uint32_t *pedge, const uint32_t *target, uint32_t *next, uint32_t *cnt)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nf) return;
    const uint32_t u = front[k], mask = wmask[comp_of[u]];
    for (uint32_t e = off[u]; e < off[u + 1]; ++e) {
        if (!(type[e] & mask)) continue;
        const uint32_t w = dst[e];
        if (__hip_atomic_load(&pedge[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kNone) continue;
        if (atomicCAS(&pedge[w], kNone, e) != kNone) continue;
        next[atomicAdd(&cnt[0], 1u)] = w;
        if (target[w]) atomicAdd(&cnt[1], 1u);
    }
}

void CoreBufs::release_core()
{
    DBuf *all[] = {&flag, &id, &node_txn, &root, &cid, &comp_of, &comp_label, &eflag, &epos, &csrc,
                   &cdst, &ctype, &coff, &f1, &fa, &s1, &e1i, &aa, &ab, &ae, &scratch};
    for (DBuf *b : all) b->release();
    e1.release_all();
}

void AnomBufs::release_all()
{
    DBuf *all[] = {&closed, &F, &B, &gs, &g1c, &cg2, &cls, &wmin, &wsrc, &wtgt, &wmask, &pedge,
                   &target, &front, &front2, &cnt};
    for (DBuf *b : all) b->release();
    release_core();
}

// graph_scc of the build, then step "core" of the header comment: the dense
// relabelling, the typed CSR of the edges inside a component, the E1 / anti
// split (f1 / fa hold their exclusive scans afterwards) and the CSR / CSC of
// (core, E1) in a.e1.  d.nc == 0: no component of >= 2 txns, nothing else set.
hipError_t graph_core(uint32_t nn, GraphBufs &g, CoreBufs &a, CoreDims &d, uint32_t *rounds,
                      uint32_t *iterations, hipStream_t s)
{
    hipError_t e = hipSuccess;
#define CK(x)                                 \
    do {                                      \
        e = (x);                              \
        if (e != hipSuccess) return e;        \
    } while (0)
    d = CoreDims{0, 0, 0, 0, 0};
    CK(graph_scc(nn, g, rounds, iterations, s));
    const uint32_t *scc = g.scc.as<uint32_t>();
    // ---- a. core: nodes ----
    CK(a.flag.ensure(4 * ((size_t)nn + 1)));
    CK(a.id.ensure(4 * ((size_t)nn + 1)));
    CK(a.scratch.ensure(scan_scratch_bytes(std::max<size_t>((size_t)nn, g.ne) + 1) + 64));
    CK(hipMemsetAsync(a.flag.p, 0, 4 * ((size_t)nn + 1), s));
    k_an_member<<<blocks(nn), 256, 0, s>>>(nn, scc, a.flag.as<uint32_t>());
    CK(hipMemcpyAsync(a.id.p, a.flag.p, 4 * ((size_t)nn + 1), hipMemcpyDeviceToDevice, s));
    CK(scan_exclusive_u32(a.id.as<uint32_t>(), (size_t)nn + 1, a.scratch.as<uint32_t>(), s));
    uint32_t nc = 0;
    CK(hipMemcpyAsync(&nc, a.id.as<uint32_t>() + nn, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    d.nc = nc;
    if (nc == 0) return hipSuccess;
    CK(a.node_txn.ensure(4 * (size_t)nc));
    CK(a.root.ensure(4 * ((size_t)nc + 1)));
    CK(a.cid.ensure(4 * ((size_t)nc + 1)));
    CK(a.comp_of.ensure(4 * (size_t)nc));
    CK(hipMemsetAsync(a.root.p, 0, 4 * ((size_t)nc + 1), s));
    k_an_nodes<<<blocks(nn), 256, 0, s>>>(nn, a.flag.as<uint32_t>(), a.id.as<uint32_t>(), scc,
                                          a.node_txn.as<uint32_t>(), a.root.as<uint32_t>());
    CK(hipMemcpyAsync(a.cid.p, a.root.p, 4 * ((size_t)nc + 1), hipMemcpyDeviceToDevice, s));
    CK(scan_exclusive_u32(a.cid.as<uint32_t>(), (size_t)nc + 1, a.scratch.as<uint32_t>(), s));
    uint32_t ncomp = 0;
    CK(hipMemcpyAsync(&ncomp, a.cid.as<uint32_t>() + nc, 4, hipMemcpyDeviceToHost, s));
    // ---- a. core: edges ----
    const size_t ne = g.ne;
    CK(a.eflag.ensure(4 * (ne + 1)));
    CK(a.epos.ensure(4 * (ne + 1)));
    if (ne)
        k_an_eflags<<<blocks(ne), 256, 0, s>>>(ne, g.src.as<uint32_t>(), g.out_dst.as<uint32_t>(), scc,
                                               a.eflag.as<uint32_t>());
    CK(hipMemsetAsync(a.eflag.as<uint32_t>() + ne, 0, 4, s));
    CK(hipMemcpyAsync(a.epos.p, a.eflag.p, 4 * (ne + 1), hipMemcpyDeviceToDevice, s));
    CK(scan_exclusive_u32(a.epos.as<uint32_t>(), ne + 1, a.scratch.as<uint32_t>(), s));
    uint32_t me = 0;
    CK(hipMemcpyAsync(&me, a.epos.as<uint32_t>() + ne, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (ncomp == 0 || me == 0) return hipErrorUnknown;  // a component of >= 2 has a root and a cycle
    CK(a.comp_label.ensure(4 * (size_t)ncomp));
    k_an_comps<<<blocks(nc), 256, 0, s>>>(nc, a.node_txn.as<uint32_t>(), scc, a.id.as<uint32_t>(),
                                          a.cid.as<uint32_t>(), a.comp_of.as<uint32_t>(),
                                          a.comp_label.as<uint32_t>());
    CK(a.csrc.ensure(4 * (size_t)me));
    CK(a.cdst.ensure(4 * (size_t)me));
    CK(a.ctype.ensure(4 * (size_t)me));
    k_an_erows<<<blocks(ne), 256, 0, s>>>(ne, g.src.as<uint32_t>(), g.out_dst.as<uint32_t>(),
                                          g.type.as<uint32_t>(), scc, a.epos.as<uint32_t>(),
                                          a.id.as<uint32_t>(), a.csrc.as<uint32_t>(), a.cdst.as<uint32_t>(),
                                          a.ctype.as<uint32_t>());
    CK(a.coff.ensure(4 * ((size_t)nc + 1)));
    k_an_offsets<<<blocks((size_t)nc + 1), 256, 0, s>>>(nc, me, a.csrc.as<uint32_t>(), a.coff.as<uint32_t>());
    // E1 rows and anti edges
    CK(a.f1.ensure(4 * ((size_t)me + 1)));
    CK(a.fa.ensure(4 * ((size_t)me + 1)));
    k_an_split_flags<<<blocks(me), 256, 0, s>>>(me, a.ctype.as<uint32_t>(), a.f1.as<uint32_t>(),
                                                a.fa.as<uint32_t>());
    CK(hipMemsetAsync(a.f1.as<uint32_t>() + me, 0, 4, s));
    CK(hipMemsetAsync(a.fa.as<uint32_t>() + me, 0, 4, s));
    CK(scan_exclusive_u32(a.f1.as<uint32_t>(), (size_t)me + 1, a.scratch.as<uint32_t>(), s));
    CK(scan_exclusive_u32(a.fa.as<uint32_t>(), (size_t)me + 1, a.scratch.as<uint32_t>(), s));
    uint32_t m1 = 0, na = 0;
    CK(hipMemcpyAsync(&m1, a.f1.as<uint32_t>() + me, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&na, a.fa.as<uint32_t>() + me, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    GraphBufs &g1 = a.e1;
    CK(a.s1.ensure(4 * ((size_t)m1 + 1)));
    CK(a.e1i.ensure(4 * ((size_t)m1 + 1)));
    CK(g1.out_dst.ensure(4 * ((size_t)m1 + 1)));
    CK(g1.in_src.ensure(4 * ((size_t)m1 + 1)));
    CK(g1.out_off.ensure(4 * ((size_t)nc + 1)));
    CK(g1.in_off.ensure(4 * ((size_t)nc + 1)));
    CK(g1.flags.ensure(4 * ((size_t)nc + 1)));  // the CSC fill's cursors
    CK(a.aa.ensure(4 * ((size_t)na + 1)));
    CK(a.ab.ensure(4 * ((size_t)na + 1)));
    CK(a.ae.ensure(4 * ((size_t)na + 1)));
    uint32_t *s1 = a.s1.as<uint32_t>(), *d1 = g1.out_dst.as<uint32_t>();
    k_an_split_rows<<<blocks(me), 256, 0, s>>>(me, a.csrc.as<uint32_t>(), a.cdst.as<uint32_t>(),
                                               a.ctype.as<uint32_t>(), a.f1.as<uint32_t>(),
                                               a.fa.as<uint32_t>(), s1, d1, a.e1i.as<uint32_t>(),
                                               a.aa.as<uint32_t>(), a.ab.as<uint32_t>(), a.ae.as<uint32_t>());
    k_an_offsets<<<blocks((size_t)nc + 1), 256, 0, s>>>(nc, m1, s1, g1.out_off.as<uint32_t>());
    CK(hipMemsetAsync(g1.in_off.p, 0, 4 * ((size_t)nc + 1), s));
    if (m1) k_an_indeg<<<blocks(m1), 256, 0, s>>>(m1, d1, g1.in_off.as<uint32_t>());
    CK(scan_exclusive_u32(g1.in_off.as<uint32_t>(), (size_t)nc + 1, a.scratch.as<uint32_t>(), s));
    CK(hipMemcpyAsync(g1.flags.p, g1.in_off.p, 4 * ((size_t)nc + 1), hipMemcpyDeviceToDevice, s));
    if (m1) k_an_infill<<<blocks(m1), 256, 0, s>>>(m1, s1, d1, g1.flags.as<uint32_t>(), g1.in_src.as<uint32_t>());
    CK(hipGetLastError());
    d.ncomp = ncomp;
    d.me = me;
    d.m1 = m1;
    d.na = na;
#undef CK
    return hipSuccess;
}

hipError_t graph_anomalies(uint32_t nn, GraphBufs &g, AnomBufs &a, bool witness, uint32_t max_batches,
                           AnomOut &out, hipStream_t s)
{
    hipError_t e = hipSuccess;
#define CK(x)                                 \
    do {                                      \
        e = (x);                              \
        if (e != hipSuccess) return e;        \
    } while (0)
    out.clear(nn);
    if (nn == 0) return hipSuccess;
    CoreDims cd;
    CK(graph_core(nn, g, a, cd, &out.scc_rounds, &out.scc_iterations, s));
    const uint32_t nc = cd.nc, ncomp = cd.ncomp, me = cd.me, m1 = cd.m1, na = cd.na;
    out.core_nodes = nc;
    if (nc == 0) return hipSuccess;
    GraphBufs &g1 = a.e1;
    uint32_t *s1 = a.s1.as<uint32_t>(), *d1 = g1.out_dst.as<uint32_t>();

    // ---- b. G1c: the components of (core, E1) ----
    uint32_t r1 = 0, i1 = 0;
    // (the colouring appends a node to its frontier once per colour it takes
    // in a step: room for a push per row on top of graph_scc's own sizing)
    CK(g1.front.ensure(4 * ((size_t)nc + m1) + 64));
    CK(g1.front2.ensure(4 * ((size_t)nc + m1) + 64));
    CK(graph_scc(nc, g1, &r1, &i1, s));
    CK(a.g1c.ensure(4 * (size_t)nc));
    CK(hipMemsetAsync(a.g1c.p, 0, 4 * (size_t)nc, s));
    k_an_member<<<blocks(nc), 256, 0, s>>>(nc, g1.scc.as<uint32_t>(), a.g1c.as<uint32_t>());

    // ---- d. G2: components holding an anti edge ----
    CK(a.cg2.ensure(4 * (size_t)ncomp));
    CK(hipMemsetAsync(a.cg2.p, 0, 4 * (size_t)ncomp, s));
    if (na) k_an_g2<<<blocks(na), 256, 0, s>>>(na, a.aa.as<uint32_t>(), a.comp_of.as<uint32_t>(), a.cg2.as<uint32_t>());

    // ---- c. G-single ----
    CK(a.gs.ensure(4 * (size_t)nc));
    CK(a.closed.ensure(4 * ((size_t)na + 1)));
    CK(a.cnt.ensure(64));
    CK(hipMemsetAsync(a.gs.p, 0, 4 * (size_t)nc, s));
    CK(hipMemsetAsync(a.closed.p, 0, 4 * ((size_t)na + 1), s));
    out.anti_edges = na;
    uint32_t nt = na;
    if (max_batches && (uint64_t)max_batches * 64 < nt) nt = max_batches * 64;
    out.anti_tested = nt;
    const uint32_t nbatch = (nt + 63) / 64;
    out.reach_batches = nbatch;
    if (nbatch) {
        // 64 batches to a launch (a wave per node) while F and B fit kReachBytes
        int lg = 6;
        while (lg > 0 && ((size_t)16 << lg) * nc > kReachBytes) --lg;
        while (lg > 0 && ((uint32_t)1 << (lg - 1)) >= nbatch) --lg;
        const uint32_t G = 1u << lg;
        const size_t total = (size_t)nc << lg;
        CK(a.F.ensure(8 * total));
        CK(a.B.ensure(8 * total));
        unsigned long long *F = a.F.as<unsigned long long>(), *B = a.B.as<unsigned long long>();
        uint32_t *chg = a.cnt.as<uint32_t>();
        for (uint32_t b0 = 0; b0 < nbatch; b0 += G) {
            const uint32_t gb = std::min(G, nbatch - b0);
            const uint32_t j0 = b0 * 64, n = std::min(nt - j0, gb * 64);
            CK(hipMemsetAsync(F, 0, 8 * total, s));
            CK(hipMemsetAsync(B, 0, 8 * total, s));
            k_an_reach_seed<<<blocks(n), 256, 0, s>>>(j0, n, lg, a.aa.as<uint32_t>(), a.ab.as<uint32_t>(), F, B);
            for (;;) {
                // kSweepsPerSync sweeps to a round trip, a change word each: the
                // first sweep that changed nothing ends the group (those after
                // it found the fixpoint again)
                uint32_t h[kSweepsPerSync];
                CK(hipMemsetAsync(chg, 0, 4 * kSweepsPerSync, s));
                for (int k = 0; k < kSweepsPerSync; ++k)
                    k_an_reach_sweep<<<blocks(total), 256, 0, s>>>(total, lg, g1.out_off.as<uint32_t>(), d1, F, B,
                                                                   chg + k);
                out.sweeps += kSweepsPerSync;
                CK(hipMemcpyAsync(h, chg, 4 * kSweepsPerSync, hipMemcpyDeviceToHost, s));
                CK(hipStreamSynchronize(s));
                bool done = false;
                for (int k = 0; k < kSweepsPerSync; ++k) done |= h[k] == 0;
                if (done) break;
                if (out.sweeps > (uint64_t)nbatch * (2 * (uint64_t)nc + 2)) return hipErrorUnknown;  // cannot happen
            }
            k_an_reach_closed<<<blocks(n), 256, 0, s>>>(j0, n, lg, a.aa.as<uint32_t>(), F, a.closed.as<uint32_t>());
            k_an_reach_mark<<<blocks(total), 256, 0, s>>>(total, lg, F, B, a.gs.as<uint32_t>());
        }
    }
    CK(a.cls.ensure(4 * (size_t)nc));
    k_an_cls<<<blocks(nc), 256, 0, s>>>(nc, a.g1c.as<uint32_t>(), a.gs.as<uint32_t>(), a.cg2.as<uint32_t>(),
                                        a.comp_of.as<uint32_t>(), a.cls.as<uint32_t>());
    CK(hipGetLastError());

    // ---- results: per txn, per component ----
    std::vector<uint32_t> node_txn(nc), cls(nc), comp_of(nc);
    out.comp_label.resize(ncomp);
    CK(hipMemcpyAsync(node_txn.data(), a.node_txn.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(cls.data(), a.cls.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(comp_of.data(), a.comp_of.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(out.comp_label.data(), a.comp_label.p, 4 * (size_t)ncomp, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    std::vector<uint8_t> cor(ncomp, 0);
    for (uint32_t u = 0; u < nc; ++u) {
        if (node_txn[u] >= nn || comp_of[u] >= ncomp) return hipErrorUnknown;
        out.cls[node_txn[u]] = (uint8_t)cls[u];
        cor[comp_of[u]] |= (uint8_t)cls[u];
        for (int k = 0; k < 3; ++k) out.txns[k] += (cls[u] >> k) & 1;
    }
    out.comp_class.resize(ncomp);
    for (uint32_t c = 0; c < ncomp; ++c) {
        if (!cor[c]) return hipErrorUnknown;  // a cycle without an anti edge is an E1 cycle
        const uint8_t k = (uint8_t)(cor[c] & (uint8_t)-cor[c]);
        out.comp_class[c] = k;
        out.comps[k == 1 ? 0 : k == 2 ? 1 : 2]++;
    }
    out.wit_off.assign((size_t)ncomp + 1, 0);
    if (!witness) return hipSuccess;

    // ---- e. witnesses ----
    CK(a.wmin.ensure(12 * (size_t)ncomp));
    CK(hipMemsetAsync(a.wmin.p, 0xFF, 12 * (size_t)ncomp, s));
    if (m1)
        k_an_wmin_e1<<<blocks(m1), 256, 0, s>>>(m1, s1, d1, a.e1i.as<uint32_t>(), g1.scc.as<uint32_t>(),
                                                a.comp_of.as<uint32_t>(), a.wmin.as<uint32_t>());
    if (na)
        k_an_wmin_anti<<<blocks(na), 256, 0, s>>>(na, a.aa.as<uint32_t>(), a.ae.as<uint32_t>(),
                                                  a.closed.as<uint32_t>(), a.comp_of.as<uint32_t>(),
                                                  a.wmin.as<uint32_t>());
    std::vector<uint32_t> wmin(3 * (size_t)ncomp), csrc(me), cdst(me), ctype(me);
    CK(hipMemcpyAsync(wmin.data(), a.wmin.p, 12 * (size_t)ncomp, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(csrc.data(), a.csrc.p, 4 * (size_t)me, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(cdst.data(), a.cdst.p, 4 * (size_t)me, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(ctype.data(), a.ctype.p, 4 * (size_t)me, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    std::vector<uint32_t> close(ncomp), wsrc(ncomp), wtgt(ncomp), wmask(ncomp);
    for (uint32_t c = 0; c < ncomp; ++c) {
        const uint8_t k = out.comp_class[c];
        const uint32_t ce = wmin[3 * (size_t)c + (k == 1 ? 0 : k == 2 ? 1 : 2)];
        if (ce >= me) return hipErrorUnknown;
        close[c] = ce;
        wsrc[c] = cdst[ce];
        wtgt[c] = csrc[ce];
        wmask[c] = k == 4 ? (kE1 | kAnti) : kE1;  // G1c / G-single paths stay on E1
    }
    CK(a.wsrc.ensure(4 * (size_t)ncomp));
    CK(a.wtgt.ensure(4 * (size_t)ncomp));
    CK(a.wmask.ensure(4 * (size_t)ncomp));
    CK(a.pedge.ensure(4 * (size_t)nc));
    CK(a.target.ensure(4 * (size_t)nc));
    CK(a.front.ensure(4 * (size_t)nc + 64));
    CK(a.front2.ensure(4 * (size_t)nc + 64));
    CK(hipMemcpyAsync(a.wsrc.p, wsrc.data(), 4 * (size_t)ncomp, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(a.wtgt.p, wtgt.data(), 4 * (size_t)ncomp, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(a.wmask.p, wmask.data(), 4 * (size_t)ncomp, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(a.pedge.p, 0xFF, 4 * (size_t)nc, s));
    CK(hipMemsetAsync(a.target.p, 0, 4 * (size_t)nc, s));
    uint32_t *cnt = a.cnt.as<uint32_t>() + 4;
    CK(hipMemsetAsync(cnt, 0, 8, s));
    k_an_bfs_init<<<blocks(ncomp), 256, 0, s>>>(ncomp, a.wsrc.as<uint32_t>(), a.wtgt.as<uint32_t>(),
                                                a.pedge.as<uint32_t>(), a.target.as<uint32_t>(),
                                                a.front.as<uint32_t>());
    uint32_t *f = a.front.as<uint32_t>(), *f2 = a.front2.as<uint32_t>();
    uint32_t nf = ncomp, found = 0;
    while (nf && found < ncomp) {
        ++out.bfs_levels;
        uint32_t h[2] = {0, 0};
        CK(hipMemsetAsync(cnt, 0, 4, s));
        k_an_bfs_step<<<blocks(nf), 256, 0, s>>>(f, nf, a.coff.as<uint32_t>(), a.cdst.as<uint32_t>(),
                                                 a.ctype.as<uint32_t>(), a.comp_of.as<uint32_t>(),
                                                 a.wmask.as<uint32_t>(), a.pedge.as<uint32_t>(),
                                                 a.target.as<uint32_t>(), f2, cnt);
        CK(hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        nf = h[0];
        found = h[1];
        if (nf > nc) return hipErrorUnknown;  // every node is claimed once
        std::swap(f, f2);
    }
    if (found < ncomp) return hipErrorUnknown;  // the closing edge lies on a cycle of its class
    std::vector<uint32_t> pedge(nc);
    CK(hipMemcpyAsync(pedge.data(), a.pedge.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    std::vector<uint32_t> rev;
    for (uint32_t c = 0; c < ncomp; ++c) {
        rev.clear();
        for (uint32_t w = wtgt[c]; w != wsrc[c];) {  // parent edges from a back to b
            const uint32_t pe = pedge[w];
            if (pe >= me || rev.size() > nc) return hipErrorUnknown;
            rev.push_back(pe);
            w = csrc[pe];
        }
        out.wit_txn.push_back(node_txn[wsrc[c]]);
        for (size_t k = rev.size(); k-- > 0;) {
            out.wit_type.push_back((uint8_t)ctype[rev[k]]);
            out.wit_txn.push_back(node_txn[cdst[rev[k]]]);
        }
        out.wit_type.push_back((uint8_t)ctype[close[c]]);
        out.wit_off[c + 1] = (uint32_t)out.wit_txn.size();
    }
#undef CK
    return hipSuccess;
}

hipError_t scc_members(uint32_t n, const uint32_t *label, uint32_t *flag, hipStream_t s)
{
    if (n) k_an_member<<<blocks(n), 256, 0, s>>>(n, label, flag);
    return hipGetLastError();
}

// load this file's code object now (see warm_graph)
hipError_t warm_anomaly()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_an_reach_sweep);
}

}  // namespace hsc
