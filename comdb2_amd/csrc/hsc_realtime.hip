// hsc_realtime.hip -- the real-time order of a history as dependency edges
// (DESIGN.md §5e): txn a precedes txn b when a completed before b was invoked,
// complete[a] < invoke[b].  With these edges (type bit kDepRT) beside ww / wr /
// rw the graph's cycles are the violations of STRICT serializability (the
// reference's linearizable/ register and bank tests ask for it); without them
// the checker answers serializability only.
//
// The full relation is quadratic and never materialised.  Its transitive
// reduction is an interval computation: with the txns sorted by (invoke, id)
// -- si[] / sc[] the invoke / complete times in that order, order[] the ids --
// and suf[p] = min(sc[p .. n)), a txn a with a closed completion c has
//     p = upper_bound(si, c)        the first txn invoked after c
//     m = suf[p]                    the first completion among those
//     q = upper_bound(si, m)        the first txn invoked after m
// and its successors are exactly order[p .. q): a txn invoked in (c, m] is
// preceded by nothing that a precedes (everything a precedes completes at m or
// later), one invoked after m follows the txn that completed at m.  An open
// completion (HSC_RT_OPEN) never lowers a minimum and has no successors.  The
// out-degree is the number of txns invoked in (c, m], all of them open at
// instant m: at most the history's concurrency.
//
// Kernels (no atomics; every cross-workgroup result crosses a kernel boundary):
//   sort     the context's radix sort (radix_sort_known) on the invoke word
//            alone, the txn id carried in the row's gid slot with its digits
//            masked out and the completion in its lsn slot: the passes are
//            stable and the input is in id order, so ties keep id order
//   suffix   two levels.  k_rt_suf_tile: the suffix minimum inside each tile of
//            kRtTile txns and the tile's minimum; k_rt_suf_top: ONE workgroup
//            turns the tile minima into exclusive suffix minima over the tiles,
//            kRtTop at a step from the last tile down, the running minimum
//            carried in a register.  suf[p] = min(in-tile[p], top[tile of p])
//            is formed where it is read, so no third pass writes it.
//   count    one thread per sorted position j: the two searches, span[j] = p
//            and cnt[j] = q - p, and the workgroup's sum as a u64 (the scan is
//            32-bit: the host checks the exact total before it sizes the rows)
//   scan     scan_exclusive_u32 over cnt
//   emit     rows order[j] << 32 | order[p + t], type kDepRT, at the scanned
//            offsets, in the staged-edge form of GraphInput (r_rows / r_type);
//            a workgroup expands its kRtThreads positions edge by edge (the
//            position of an edge searched in LDS), so the rows leave in whole
//            lines (one thread per txn writing its own run measured 2.0 ms a
//            call at 16.7 M txns, averaged over 54 M and 162 M edges; this
//            form 0.27 and 0.71 ms)
//
// The searches are plain per-thread binary searches, not the 16-lane
// cooperative search of k_probe_narrow: neighbouring threads hold neighbouring
// completions (completion order follows invoke order to within the
// concurrency), so a wave's 64 searches walk the same lines of si[] and the
// last steps hit one or two lines; §5e has the measured times.
//
// The sharded path (hsc_multi_graph_scc) exchanges untyped cut rows and takes
// no real-time edges.
#include "hsc_device.h"
#include "hsc_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>

namespace hsc {

namespace {

constexpr int kRtThreads = 256;
constexpr uint32_t kRtTile = 256;  // txns per suffix tile (one per thread)
constexpr uint32_t kRtTop = 256;   // tile minima per step of k_rt_suf_top
constexpr uint64_t kOpen = ~0ull;  // HSC_RT_OPEN

inline unsigned blocks(size_t n) { return (unsigned)((n + kRtThreads - 1) / kRtThreads); }

__global__ void k_rt_iota(uint32_t n, uint32_t *id)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) id[i] = i;
}

// Inclusive suffix minimum of one value per thread over a workgroup of
// kRtThreads: x = min over the threads >= this one; total = the workgroup's.
__device__ __forceinline__ uint64_t block_suffix_min(uint64_t v, uint64_t *lds, uint64_t &total)
{
    constexpr int NW = kRtThreads / 64;
    const int lane = lane_id(), wid = threadIdx.x >> 6;
    uint64_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t y = __shfl_down(x, o, 64);
        if (lane + o < 64 && y < x) x = y;
    }
    if (lane == 0) lds[wid] = x;
    __syncthreads();
    uint64_t later = kOpen, all = kOpen;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint64_t t = lds[w];
        if (w > wid && t < later) later = t;
        if (t < all) all = t;
    }
    __syncthreads();
    total = all;
    return later < x ? later : x;
}

// tile[i] = min(sc[i .. end of i's tile)); tmin[b] = tile b's minimum
__global__ __launch_bounds__(kRtThreads) void k_rt_suf_tile(uint32_t n, const uint64_t *sc, uint64_t *tile,
                                                            uint64_t *tmin)
{
    __shared__ uint64_t lds[kRtThreads / 64];
    const uint32_t i = blockIdx.x * kRtTile + threadIdx.x;
    uint64_t all;
    const uint64_t x = block_suffix_min(i < n ? sc[i] : kOpen, lds, all);
    if (i < n) tile[i] = x;
    if (threadIdx.x == 0) tmin[blockIdx.x] = all;
}

// top[b] = min(tmin[b + 1 .. nb)) (kOpen for the last tile); one workgroup
__global__ __launch_bounds__(kRtThreads) void k_rt_suf_top(uint32_t nb, const uint64_t *tmin, uint64_t *top)
{
    __shared__ uint64_t lds[kRtThreads / 64];
    __shared__ uint64_t first[kRtThreads / 64 + 1];  // each wave's first inclusive value, then kOpen
    uint64_t carry = kOpen;  // min of every step already done (the tiles after this step's)
    for (uint32_t step = (nb + kRtTop - 1) / kRtTop; step-- > 0;) {
        const uint32_t b = step * kRtTop + threadIdx.x;
        const uint64_t v = b < nb ? tmin[b] : kOpen;
        uint64_t all;
        const uint64_t incl = block_suffix_min(v, lds, all);
        // exclusive: the inclusive value of the next thread
        const uint64_t nxt = __shfl_down(incl, 1, 64);
        if (lane_id() == 0) first[threadIdx.x >> 6] = incl;
        if (threadIdx.x == 0) first[kRtThreads / 64] = kOpen;
        __syncthreads();
        const uint64_t excl = lane_id() == 63 ? first[(threadIdx.x >> 6) + 1] : nxt;
        if (b < nb) top[b] = excl < carry ? excl : carry;
        if (all < carry) carry = all;
        __syncthreads();
    }
}

// first index in [lo, n) with si[index] > x (si sorted)
__device__ __forceinline__ uint32_t upper_from(const uint64_t *si, uint32_t lo, uint32_t n, uint64_t x)
{
    uint32_t len = n - lo;
    while (len > 0) {
        const uint32_t half = len >> 1, mid = lo + half;
        if (si[mid] <= x) {
            lo = mid + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return lo;
}

// span[j] = p, cnt[j] = q - p of the txn at sorted position j; bsum[block] =
// the workgroup's edges
__global__ __launch_bounds__(kRtThreads) void k_rt_count(uint32_t n, const uint64_t *si, const uint64_t *sc,
                                                         const uint64_t *tile, const uint64_t *top, uint32_t *span,
                                                         uint32_t *cnt, uint64_t *bsum)
{
    __shared__ uint64_t lds[kRtThreads / 64];
    const uint32_t j = blockIdx.x * kRtThreads + threadIdx.x;
    uint32_t p = 0, k = 0;
    if (j < n) {
        const uint64_t c = sc[j];
        if (c != kOpen) {
            p = upper_from(si, j + 1, n, c);  // si[j] <= c: the search starts past j
            if (p < n) {
                const uint64_t a = tile[p], b = top[p / kRtTile];
                const uint64_t m = a < b ? a : b;
                k = upper_from(si, p, n, m) - p;
            }
        }
        span[j] = p;
        cnt[j] = k;
    }
    uint64_t x = k;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int w = 0; w < kRtThreads / 64; ++w) t += lds[w];
        bsum[blockIdx.x] = t;
    }
}

// total[0] = sum of bsum[0 .. nb); one workgroup
__global__ __launch_bounds__(1024) void k_rt_total(uint32_t nb, const uint64_t *bsum, uint64_t *total)
{
    __shared__ uint64_t lds[1024 / 64];
    uint64_t x = 0;
    for (uint32_t i = threadIdx.x; i < nb; i += 1024) x += bsum[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t = 0;
        for (int w = 0; w < 1024 / 64; ++w) t += lds[w];
        total[0] = t;
    }
}

// off = the exclusive scan of cnt (off[n] = total).  A workgroup takes the
// edges of its kRtThreads sorted positions, one edge per thread and step: the
// edge's position is found among the workgroup's offsets in LDS, so the rows
// are written (and the successors' ids read) in whole lines whatever the
// out-degrees are.
__global__ __launch_bounds__(kRtThreads) void k_rt_emit(uint32_t n, const uint32_t *id, const uint32_t *span,
                                                        const uint32_t *off, uint32_t total, uint64_t *rows,
                                                        uint64_t *type)
{
    __shared__ uint32_t loff[kRtThreads + 1], lspan[kRtThreads], lid[kRtThreads];
    const uint32_t j0 = blockIdx.x * kRtThreads, j = j0 + threadIdx.x;
    loff[threadIdx.x] = min(off[min(j, n)], total);
    if (threadIdx.x == 0) loff[kRtThreads] = min(off[min(j0 + kRtThreads, n)], total);
    lspan[threadIdx.x] = j < n ? span[j] : 0;
    lid[threadIdx.x] = j < n ? id[j] : 0;
    __syncthreads();
    const uint32_t e1 = loff[kRtThreads];
    for (uint32_t e = loff[0] + threadIdx.x; e < e1; e += kRtThreads) {
        uint32_t lo = 0, len = kRtThreads;  // the last position whose offset is <= e
        while (len > 1) {
            const uint32_t half = len >> 1;
            if (loff[lo + half] <= e) lo += half;
            len -= half;
        }
        const uint32_t b = lspan[lo] + (e - loff[lo]);
        if (b >= n) continue;  // (cnt never reaches past the last txn)
        rows[e] = ((uint64_t)lid[lo] << 32) | id[b];
        type[e] = kDepRT;
    }
}

}  // namespace

hipError_t realtime_stage(uint32_t n, const uint64_t *invoke, const uint64_t *complete, GraphBufs &g,
                          hipStream_t s)
{
    hipError_t e = hipSuccess;
#define CK(x)                                 \
    do {                                      \
        e = (x);                              \
        if (e != hipSuccess) return e;        \
    } while (0)
    g.n_rt = 0;
    g.rt_ntxn = n;
    if (n == 0) return hipSuccess;
    const size_t cap = ((size_t)n + 63) & ~(size_t)63;
    const uint32_t nb = (n + kRtTile - 1) / kRtTile;
    for (DBuf *b : {&g.rt_inv, &g.rt_cpl, &g.rt_inv2, &g.rt_cpl2, &g.rt_suf}) CK(b->ensure(8 * cap));
    for (DBuf *b : {&g.rt_id, &g.rt_id2, &g.rt_span}) CK(b->ensure(4 * cap));
    CK(g.rt_cnt.ensure(4 * (cap + 64)));
    CK(g.rt_bmin.ensure(8 * 2 * (size_t)nb));
    CK(g.rt_sum.ensure(8 * ((size_t)nb + 1)));
    CK(g.scratch.ensure(std::max(radix_scratch_bytes(n, 1), scan_scratch_bytes((size_t)n + 1) + 64)));
    CK(hipMemcpyAsync(g.rt_inv.p, invoke, 8 * (size_t)n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(g.rt_cpl.p, complete, 8 * (size_t)n, hipMemcpyHostToDevice, s));
    k_rt_iota<<<blocks(n), kRtThreads, 0, s>>>(n, g.rt_id.as<uint32_t>());
    CK(hipGetLastError());
    // the invoke word's varying bits; the id (the row's gid slot) is carried, never a digit
    uint64_t vary[2] = {0, 0};
    CK(vary_mask_rows(1, n, g.rt_id.as<uint32_t>(), g.rt_inv.as<uint64_t>(), cap, g.scratch.p, vary, s));
    vary[1] = 0;
    bool alt = false;
    CK(radix_sort_known(1, n, g.rt_id.as<uint32_t>(), g.rt_inv.as<uint64_t>(), g.rt_cpl.as<uint64_t>(), cap,
                        g.rt_id2.as<uint32_t>(), g.rt_inv2.as<uint64_t>(), g.rt_cpl2.as<uint64_t>(),
                        g.scratch.p, g.scratch.bytes, &alt, vary, s));
    const uint32_t *id = alt ? g.rt_id2.as<uint32_t>() : g.rt_id.as<uint32_t>();
    const uint64_t *si = alt ? g.rt_inv2.as<uint64_t>() : g.rt_inv.as<uint64_t>();
    const uint64_t *sc = alt ? g.rt_cpl2.as<uint64_t>() : g.rt_cpl.as<uint64_t>();
    uint64_t *tmin = g.rt_bmin.as<uint64_t>(), *top = tmin + nb;
    k_rt_suf_tile<<<nb, kRtThreads, 0, s>>>(n, sc, g.rt_suf.as<uint64_t>(), tmin);
    k_rt_suf_top<<<1, kRtThreads, 0, s>>>(nb, tmin, top);
    uint32_t *cnt = g.rt_cnt.as<uint32_t>();
    uint64_t *bsum = g.rt_sum.as<uint64_t>();
    k_rt_count<<<nb, kRtThreads, 0, s>>>(n, si, sc, g.rt_suf.as<uint64_t>(), top, g.rt_span.as<uint32_t>(), cnt,
                                        bsum);
    k_rt_total<<<1, 1024, 0, s>>>(nb, bsum, bsum + nb);
    CK(hipGetLastError());
    CK(hipMemsetAsync(cnt + n, 0, 4, s));
    uint64_t total = 0;
    CK(hipMemcpyAsync(&total, bsum + nb, 8, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (total > kRtMaxEdges) return hipErrorInvalidValue;
    if (total == 0) return hipSuccess;
    CK(g.rt_rows.ensure(8 * (size_t)total));
    CK(g.rt_type.ensure(8 * (size_t)total));
    CK(scan_exclusive_u32(cnt, (size_t)n + 1, g.scratch.as<uint32_t>(), s));
    k_rt_emit<<<nb, kRtThreads, 0, s>>>(n, id, g.rt_span.as<uint32_t>(), cnt, (uint32_t)total,
                                       g.rt_rows.as<uint64_t>(), g.rt_type.as<uint64_t>());
    CK(hipGetLastError());
    g.n_rt = (size_t)total;
#undef CK
    return hipSuccess;
}

// load this file's code object now (see warm_graph)
hipError_t warm_realtime()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_rt_count);
}

}  // namespace hsc
