// hsc_intcons.hip -- internal consistency (Elle's :internal):
// every read of a txn against that txn's own earlier ops on the key.  A pure
// function of the history the last resolve of its kind left on the device
// (ResolveBufs::in_* / ListBufs::in_*): nothing is uploaded, and nothing the
// resolve left for the build is written.
//
// Passes (the discipline of hsc_resolve.hip: flag + scan_exclusive_u32
// compaction, so every output keeps op order; a plain store of 1 wherever one
// does; the only atomics are the counters, one per workgroup and counter that
// is not zero):
//   rows      one row (txn, key) per op with the op as payload, in op order
//   sort      sort_rows2, stable: inside an equal run the ops of one (txn, key)
//             stand in program order
//   value     (value histories) one thread per sorted position: a read whose
//             left neighbour has its (txn, key) is constrained, its anchor that
//             neighbour, bad iff the two values differ
//   bounds    (list histories) a boundary is a sorted position that heads a run
//             or is a read; flags, scan, positions compacted: the boundary left
//             of a read at q is its previous read p, or the run's head append
//             when there is none, and the appends between are the sorted
//             positions in between -- the j-th expected appended element is one
//             load away
//   reads     (list histories) per sorted position: anchor, the length
//             condition (a read that fails it is bad and compares nothing), the
//             elements to compare and their number of chunks of kIcChunk
//   compare   (list histories) the chunk counts scanned enumerate the (read,
//             chunk) items; one wave per item, the lanes stride the chunk with
//             8-byte loads of the read's elements and of the previous read's
//             or the appended values; a mismatch is a plain store of 1
//   counts    the constrained / bad reads of counted txns, the per-txn plane,
//             the listed reads compacted up to the cap with their anchors
#include <algorithm>

#include "hsc_internal.h"
#include "hsc_table_dev.h"

namespace hsc {

namespace {

constexpr uint64_t kIcNone = ~0ull;
constexpr int kIcChunkLog2 = 10;
constexpr uint32_t kIcChunk = 1u << kIcChunkLog2;  // elements one wave compares
enum { kIcChecked, kIcBad, kIcCompared, kIcBadTxns, kIcN };

inline unsigned ic_blocks(size_t n) { return (unsigned)((n + kRvThreads - 1) / kRvThreads); }

__global__ __launch_bounds__(kRvThreads) void k_ic_rows(size_t nops, const uint32_t *txn, const uint64_t *key,
                                                        size_t cap, uint64_t *rows, uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= nops) return;
    rows[i] = txn[i];
    rows[cap + i] = key[i];
    pay[i] = i;
}

// the sorted position q (> 0) continues its left neighbour's (txn, key) run
__device__ __forceinline__ bool ic_same(const uint64_t *ws, size_t cap, size_t q)
{
    return ws[q] == ws[q - 1] && ws[cap + q] == ws[cap + q - 1];
}

__global__ __launch_bounds__(kRvThreads) void k_ic_value(size_t nops, const uint64_t *ws, size_t cap,
                                                         const uint64_t *ps, const uint8_t *isw,
                                                         const uint64_t *value, uint8_t *bad, uint64_t *anchor)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q >= nops) return;
    const uint64_t op = ps[q];
    uint64_t a = kIcNone;
    uint8_t b = 0;
    if (!isw[op] && q > 0 && ic_same(ws, cap, q)) {
        a = ps[q - 1];
        b = value[op] != value[a];
    }
    anchor[op] = a;
    bad[op] = b;
}

__global__ __launch_bounds__(kRvThreads) void k_ic_bflag(size_t nops, const uint64_t *ws, size_t cap,
                                                         const uint64_t *ps, const uint8_t *isw, uint32_t *bflag)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > nops) return;
    bflag[q] = q < nops && (q == 0 || !ic_same(ws, cap, q) || !isw[ps[q]]);
}

// bs: the exclusive scan of the boundary flags
__global__ __launch_bounds__(kRvThreads) void k_ic_bpos(size_t nops, const uint32_t *bs, uint32_t *bpos)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q >= nops) return;
    const uint32_t x = bs[q];
    if (bs[q + 1] != x) bpos[x] = (uint32_t)q;
}

// What a constrained list read at sorted position q (not a run head) compares:
// cnt elements of its list from element `from`, the first `lenp` against the
// previous read's list at offp, the rest against the appended values of the
// sorted positions from `at`.  ok: the length condition.
struct IcRead {
    uint64_t anchor, offj, offp;
    uint32_t from, lenp, cnt, at;
    bool ok;
};
__device__ __forceinline__ IcRead ic_read(size_t q, uint64_t op, const uint64_t *ps, const uint32_t *bs,
                                          const uint32_t *bpos, const uint8_t *isw, const uint64_t *off)
{
    IcRead r;
    const uint32_t b = bpos[bs[q] - 1];  // the boundary left of q: inside the run, whose head is one
    const uint64_t pb = ps[b];
    const uint32_t lenj = (uint32_t)(off[op + 1] - off[op]);
    r.anchor = pb;
    r.offj = off[op];
    if (!isw[pb]) {  // the previous read p; the appends between stand at b + 1 .. q - 1
        const uint32_t a = (uint32_t)q - 1 - b;
        r.offp = off[pb];
        r.lenp = (uint32_t)(off[pb + 1] - r.offp);
        r.ok = lenj == r.lenp + a;
        r.from = 0;
        r.cnt = lenj;
        r.at = b + 1;
    } else {  // no read before: the run's appends b .. q - 1 are the list's tail
        const uint32_t a = (uint32_t)q - b;
        r.offp = 0;
        r.lenp = 0;
        r.ok = lenj >= a;
        r.from = lenj - a;
        r.cnt = a;
        r.at = b;
    }
    return r;
}

__global__ __launch_bounds__(kRvThreads) void k_ic_reads(size_t nops, const uint64_t *ws, size_t cap,
                                                         const uint64_t *ps, const uint32_t *bs,
                                                         const uint32_t *bpos, const uint32_t *txn,
                                                         const uint8_t *isw, const uint64_t *off,
                                                         const uint8_t *status, uint8_t *bad, uint64_t *anchor,
                                                         uint32_t *chunks, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][1];
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[1] = {0};
    if (q < nops) {
        const uint64_t op = ps[q];
        uint64_t a = kIcNone;
        uint8_t b = 0;
        uint32_t nch = 0;
        if (!isw[op] && q > 0 && ic_same(ws, cap, q) && status[txn[op]] == HSC_TXN_OK) {
            const IcRead r = ic_read(q, op, ps, bs, bpos, isw, off);
            a = r.anchor;
            b = !r.ok;
            if (r.ok) {
                v[0] = r.cnt;  // (their sum is at most the history's elements: below 2^31)
                nch = (r.cnt + kIcChunk - 1) >> kIcChunkLog2;
            }
        }
        anchor[op] = a;
        bad[op] = b;
        chunks[q] = nch;
    } else if (q == nops) {
        chunks[q] = 0;
    }
    block_add<1>(v, ct + kIcCompared, lds);
}

// cs: the exclusive scan of the chunk counts, cs[nops] = items; one wave per item
__global__ __launch_bounds__(kRvThreads) void k_ic_compare(uint32_t items, size_t nops, const uint32_t *cs,
                                                           const uint64_t *ps, const uint32_t *bs,
                                                           const uint32_t *bpos, const uint8_t *isw,
                                                           const uint64_t *value, const uint64_t *off,
                                                           const uint64_t *elems, uint8_t *bad)
{
    const uint32_t w = blockIdx.x * (kRvThreads / 64) + (threadIdx.x >> 6);
    if (w >= items) return;
    size_t lo = 0, hi = nops;  // the first position whose items start after w (cs[nops] = items > w)
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (cs[mid] <= w)
            lo = mid + 1;
        else
            hi = mid;
    }
    const size_t q = lo - 1;  // (cs[0] == 0 <= w)
    const uint64_t op = ps[q];
    const IcRead r = ic_read(q, op, ps, bs, bpos, isw, off);
    const uint32_t e0 = (w - cs[q]) << kIcChunkLog2, e1 = min(r.cnt, e0 + kIcChunk);
    const uint64_t *mine = elems + r.offj + r.from, *prev = elems + r.offp;
    bool mis = false;
    for (uint32_t e = e0 + lane_id(); e < e1; e += 64) {
        const uint64_t want = e < r.lenp ? prev[e] : value[ps[r.at + (e - r.lenp)]];
        mis |= mine[e] != want;
    }
    if (__ballot(mis) != 0 && lane_id() == 0) bad[op] = 1;
}

// level: the resolve's membership of C (null: every constrained read counts --
// the list entry constrains reads of OK txns only)
__global__ __launch_bounds__(kRvThreads) void k_ic_count(size_t nops, const uint32_t *txn, const uint64_t *anchor,
                                                         const uint8_t *bad, const uint32_t *level, uint8_t *plane,
                                                         uint32_t *listed, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][2];
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[2] = {0, 0};
    if (i < nops) {
        const uint32_t t = txn[i];
        const bool con = anchor[i] != kIcNone && (!level || level[t] != 0);
        const bool b = con && bad[i];
        v[0] = con;
        v[1] = b;
        if (b) plane[t] = 1;
        listed[i] = b;
    } else if (i == nops) {
        listed[i] = 0;
    }
    block_add<2>(v, ct + kIcChecked, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_ic_txns(uint32_t ntxn, const uint8_t *plane, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][1];
    const uint32_t t = blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[1] = {t < ntxn && plane[t] != 0};
    block_add<1>(v, ct + kIcBadTxns, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_ic_list(size_t nops, const uint32_t *pos, const uint64_t *anchor,
                                                        uint32_t cap, uint64_t *list_op, uint64_t *list_anchor)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= nops) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p || p >= cap) return;
    list_op[p] = i;
    list_anchor[p] = anchor[i];
}

}  // namespace

void InternalBufs::release_all()
{
    DBuf *all[] = {&rows, &pay, &bad, &anchor, &f0, &f1, &bpos, &plane, &ct, &list_op, &list_anchor};
    for (DBuf *b : all) b->release();
}

#define CK(x)                          \
    do {                               \
        hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return e_; \
    } while (0)

hipError_t graph_internal(const InternalIn &in, ResolveBufs &r, InternalBufs &b, bool arrays, InternalOut &o,
                          hipStream_t s)
{
    const size_t n = in.nops;
    const uint32_t nt = in.ntxn;
    o = InternalOut{};
    o.nops = n;
    o.ntxn = nt;
    o.txn_bad.assign(nt, 0);
    if (!n) return hipSuccess;
    const size_t t1 = std::max<size_t>(nt, 1);
    CK(b.rows.ensure(8 * 2 * n));
    CK(b.pay.ensure(8 * n));
    CK(b.bad.ensure(n));
    CK(b.anchor.ensure(8 * n));
    CK(b.f0.ensure(4 * (n + 1)));
    CK(b.plane.ensure(t1));
    CK(b.ct.ensure(8 * kIcN));
    CK(b.list_op.ensure(8 * HSC_INTERNAL_LIST_CAP));
    CK(b.list_anchor.ensure(8 * HSC_INTERNAL_LIST_CAP));
    // the sort's alternates and scratch are the resolve's (sort_rows2)
    CK(r.words2.ensure(8 * 2 * n));
    CK(r.pay2.ensure(8 * n));
    CK(r.gid.ensure(4 * n));
    CK(r.gid2.ensure(4 * n));
    CK(r.k0.ensure(8 * n));
    CK(r.k1.ensure(8 * n));
    CK(r.words_dev.ensure(256));
    CK(r.scratch.ensure(std::max(std::max(radix_scratch_bytes(n, 2), packed_scratch_bytes(n)),
                                 scan_scratch_bytes(n + 2) + 64)));
    uint64_t *rows = b.rows.as<uint64_t>(), *pay = b.pay.as<uint64_t>(), *anchor = b.anchor.as<uint64_t>();
    uint8_t *bad = b.bad.as<uint8_t>(), *plane = b.plane.as<uint8_t>();
    uint32_t *f0 = b.f0.as<uint32_t>(), *scratch = nullptr;
    unsigned long long *ct = (unsigned long long *)b.ct.p;
    CK(hipMemsetAsync(ct, 0, 8 * kIcN, s));
    CK(hipMemsetAsync(plane, 0, t1, s));
    k_ic_rows<<<ic_blocks(n), kRvThreads, 0, s>>>(n, in.txn, in.key, n, rows, pay);
    CK(hipGetLastError());
    const uint64_t *ws, *ps;
    bool pk = false;
    CK(sort_rows2(n, n, r, rows, pay, &pk, &ws, &ps, s));
    o.sort_packed = pk;
    scratch = r.scratch.as<uint32_t>();
    if (!in.lists) {
        k_ic_value<<<ic_blocks(n), kRvThreads, 0, s>>>(n, ws, n, ps, in.isw, in.value, bad, anchor);
        CK(hipGetLastError());
    } else {
        CK(b.f1.ensure(4 * (n + 1)));
        CK(b.bpos.ensure(4 * n));
        uint32_t *f1 = b.f1.as<uint32_t>(), *bpos = b.bpos.as<uint32_t>();
        k_ic_bflag<<<ic_blocks(n + 1), kRvThreads, 0, s>>>(n, ws, n, ps, in.isw, f0);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(f0, n + 1, scratch, s));
        k_ic_bpos<<<ic_blocks(n), kRvThreads, 0, s>>>(n, f0, bpos);
        CK(hipGetLastError());
        k_ic_reads<<<ic_blocks(n + 1), kRvThreads, 0, s>>>(n, ws, n, ps, f0, bpos, in.txn, in.isw, in.off,
                                                           in.status, bad, anchor, f1, ct);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(f1, n + 1, scratch, s));
        uint32_t items = 0;
        CK(hipMemcpyAsync(&items, f1 + n, 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        if (items) {
            const unsigned wpb = kRvThreads / 64;
            k_ic_compare<<<(items + wpb - 1) / wpb, kRvThreads, 0, s>>>(items, n, f1, ps, f0, bpos, in.isw,
                                                                        in.value, in.off, in.elems, bad);
            CK(hipGetLastError());
        }
    }
    // counts and the listed reads (f0 now the listed flags)
    k_ic_count<<<ic_blocks(n + 1), kRvThreads, 0, s>>>(n, in.txn, anchor, bad, in.level, plane, f0, ct);
    CK(hipGetLastError());
    k_ic_txns<<<ic_blocks(t1), kRvThreads, 0, s>>>(nt, plane, ct);
    CK(hipGetLastError());
    CK(scan_exclusive_u32(f0, n + 1, scratch, s));
    k_ic_list<<<ic_blocks(n), kRvThreads, 0, s>>>(n, f0, anchor, HSC_INTERNAL_LIST_CAP, b.list_op.as<uint64_t>(),
                                                  b.list_anchor.as<uint64_t>());
    CK(hipGetLastError());
    unsigned long long hct[kIcN] = {};
    CK(hipMemcpyAsync(hct, ct, 8 * kIcN, hipMemcpyDeviceToHost, s));
    if (nt) CK(hipMemcpyAsync(o.txn_bad.data(), plane, nt, hipMemcpyDeviceToHost, s));
    if (arrays) {
        o.bad.resize(n);
        o.anchor_op.resize(n);
        CK(hipMemcpyAsync(o.bad.data(), bad, n, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.anchor_op.data(), anchor, 8 * n, hipMemcpyDeviceToHost, s));
    }
    CK(hipStreamSynchronize(s));
    o.checked_reads = hct[kIcChecked];
    o.bad_reads = hct[kIcBad];
    o.compared_elements = hct[kIcCompared];
    o.bad_txns = (uint32_t)hct[kIcBadTxns];
    o.n_listed = (uint32_t)std::min<uint64_t>(o.bad_reads, HSC_INTERNAL_LIST_CAP);
    o.listed_op.assign(o.n_listed, 0);
    o.listed_anchor.assign(o.n_listed, 0);
    if (o.n_listed) {
        CK(hipMemcpyAsync(o.listed_op.data(), b.list_op.p, 8 * (size_t)o.n_listed, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.listed_anchor.data(), b.list_anchor.p, 8 * (size_t)o.n_listed, hipMemcpyDeviceToHost,
                          s));
        CK(hipStreamSynchronize(s));
    }
    return hipSuccess;
}
#undef CK

// load this file's code object now (see warm_graph)
hipError_t warm_internal()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_ic_rows);
}

}  // namespace hsc
