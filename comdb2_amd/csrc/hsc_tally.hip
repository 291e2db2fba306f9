// hsc_tally.hip -- the accounting checkers of the reference's Jepsen suite
// (DESIGN.md §5k): checker/set and checker/total-queue as one tally of three
// value arrays, and the bank checker's per-read length and total.  Neither is a
// graph or a search.
//
// Tally passes (the discipline of hsc_resolve.hip and hsc_intcons.hip: flag +
// scan_exclusive_u32 compaction, so every output keeps ascending order; plain
// stores; the only atomics are the counters, one per workgroup and counter that
// is not zero):
//   rows      one row (value ^ sign bit, source) per element -- unsigned order
//             of the first word is signed order of the values; source 0 attempt,
//             1 ack, 2 seen
//   sort      sort_rows2 through a private set of sort rows (TallyBufs::t)
//   heads     flags of the (value, source) sub-run heads and of the value run
//             heads, both scanned; their positions compacted.  A sub-run's
//             length is the distance to the next head, so one value that occurs
//             a million times costs no thread a loop
//   classes   per distinct value the counts A, K, S of its (at most three)
//             sub-runs, clamped to 1 in set mode; the class multiplicities are
//             tl_mult below, one rule for both checkers
//   runs      per class the flags of the run heads (a run: consecutive integer
//             values of one non-zero multiplicity), all five classes scanned in
//             one array; the k-th head writes lo and mult, the k-th tail -- it
//             knows k from the same scan -- writes hi, up to the cap
//   counts    per class count / distinct / runs, per source its total, exact
//             whatever the cap
//
// Bank: one kernel, one read per group of G lanes (G a power of two from the
// model's n, at most 64), the group strides the read's balances and reduces the
// wrapping sum and the negatives by cross-lane shuffles; the bad reads' indices
// compacted in read order by flag + scan.
#include <algorithm>

#include "hsc_internal.h"
#include "hsc_table_dev.h"

namespace hsc {

namespace {

constexpr uint64_t kTlSign = 1ull << 63;
// counters: per class count and distinct, per source its total (k_tl_class adds these in one go), per class runs
enum { kTlCount = 0, kTlDistinct = HSC_TALLY_NCLASS, kTlTotal = 2 * HSC_TALLY_NCLASS,
       kTlRuns = 2 * HSC_TALLY_NCLASS + 3, kTlN = 3 * HSC_TALLY_NCLASS + 3 };
enum { kBkBad, kBkWrongN, kBkWrongTotal, kBkNegative, kBkN };

inline unsigned tl_blocks(size_t n) { return (unsigned)((n + kRvThreads - 1) / kRvThreads); }

// in: attempt | ack | seen
__global__ __launch_bounds__(kRvThreads) void k_tl_rows(size_t n, size_t n_attempt, size_t n_ack, const uint64_t *in,
                                                        size_t cap, uint64_t *rows, uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= n) return;
    rows[i] = in[i] ^ kTlSign;
    rows[cap + i] = i < n_attempt ? 0 : i < n_attempt + n_ack ? 1 : 2;
    pay[i] = i;
}

// sub[q] / run[q] (q <= n; 0 at n): the sorted position q heads a (value, source) sub-run / a value run
__global__ __launch_bounds__(kRvThreads) void k_tl_heads(size_t n, const uint64_t *ws, size_t cap, uint32_t *sub,
                                                         uint32_t *run)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > n) return;
    const bool in = q < n, nv = in && (q == 0 || ws[q] != ws[q - 1]);
    sub[q] = nv || (in && ws[cap + q] != ws[cap + q - 1]);
    run[q] = nv;
}

// sub / run scanned: spos[k] = the k-th sub-run's first position (spos[nsub] = n),
// vsub[j] = the j-th value's first sub-run (vsub[d] = nsub)
__global__ __launch_bounds__(kRvThreads) void k_tl_pos(size_t n, const uint32_t *sub, const uint32_t *run,
                                                       uint32_t *spos, uint32_t *vsub)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > n) return;
    const uint32_t s = sub[q], r = run[q];
    if (q == n) {
        spos[s] = (uint32_t)n;
        vsub[r] = s;
        return;
    }
    if (sub[q + 1] != s) spos[s] = (uint32_t)q;
    if (run[q + 1] != r) vsub[r] = s;
}

// The class multiplicities of a value with A attempts, K acks, S seen
// (jepsen/checker.clj:133-144 with every count clamped to 1, :184-207 as they are).
__device__ __forceinline__ uint32_t tl_mult(int c, uint32_t A, uint32_t K, uint32_t S)
{
    const uint32_t ok = min(S, A);
    switch (c) {
    case HSC_TALLY_OK: return ok;
    case HSC_TALLY_UNEXPECTED: return A ? 0 : S;
    case HSC_TALLY_DUPLICATED: return A && S > A ? S - A : 0;
    case HSC_TALLY_LOST: return K > S ? K - S : 0;
    default: return ok > K ? ok - K : 0;  // HSC_TALLY_RECOVERED
    }
}

// cnt: [3][dcap] A, K, S per distinct value
__global__ __launch_bounds__(kRvThreads) void k_tl_class(uint32_t d, const uint64_t *ws, size_t cap,
                                                         const uint32_t *spos, const uint32_t *vsub, int multiset,
                                                         size_t dcap, int64_t *val, uint32_t *cnt,
                                                         unsigned long long *ct)
{
    constexpr int NC = HSC_TALLY_NCLASS;
    __shared__ uint32_t lds[kRvThreads / 64][2 * NC + 3];
    const uint32_t j = blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[2 * NC + 3] = {};
    if (j < d) {
        const uint32_t s0 = vsub[j], s1 = vsub[j + 1];
        uint32_t a[3] = {0, 0, 0};
        for (uint32_t s = s0; s < s1; ++s) {  // at most three
            const uint32_t p = spos[s], len = spos[s + 1] - p;
            const uint64_t src = ws[cap + p];
            a[0] = src == 0 ? len : a[0];
            a[1] = src == 1 ? len : a[1];
            a[2] = src == 2 ? len : a[2];
        }
        if (!multiset)
            for (int k = 0; k < 3; ++k) a[k] = min(a[k], 1u);
        val[j] = (int64_t)(ws[spos[s0]] ^ kTlSign);
        for (int k = 0; k < 3; ++k) {
            cnt[k * dcap + j] = a[k];
            v[2 * NC + k] = a[k];
        }
        for (int c = 0; c < NC; ++c) {
            const uint32_t m = tl_mult(c, a[0], a[1], a[2]);
            v[c] = m;
            v[NC + c] = m != 0;
        }
    }
    // (every sum is at most the rows of the call, below 2^31)
    block_add<2 * NC + 3>(v, ct + kTlCount, lds);
}

// value j (m = its multiplicity in the class, not zero) continues the run of value j - 1 / is continued by j + 1
__device__ __forceinline__ bool tl_joined(int c, const int64_t *val, const uint32_t *cnt, size_t dcap, uint32_t lo,
                                          uint32_t m)
{
    const int64_t a = val[lo];
    return a != INT64_MAX && a + 1 == val[lo + 1] &&
           tl_mult(c, cnt[lo], cnt[dcap + lo], cnt[2 * dcap + lo]) == m &&
           tl_mult(c, cnt[lo + 1], cnt[dcap + lo + 1], cnt[2 * dcap + lo + 1]) == m;
}

// rf: [NCLASS][d + 1] the run head flags (0 at d); blockIdx.y = the class
__global__ __launch_bounds__(kRvThreads) void k_tl_runflags(uint32_t d, const int64_t *val, const uint32_t *cnt,
                                                            size_t dcap, uint32_t *rf, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][1];
    const int c = blockIdx.y;
    const uint32_t j = blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[1] = {0};
    if (j <= d) {
        if (j < d) {
            const uint32_t m = tl_mult(c, cnt[j], cnt[dcap + j], cnt[2 * dcap + j]);
            v[0] = m != 0 && !(j > 0 && tl_joined(c, val, cnt, dcap, j - 1, m));
        }
        rf[(size_t)c * ((size_t)d + 1) + j] = v[0];
    }
    block_add<1>(v, ct + kTlRuns + c, lds);
}

// rf scanned as one array: the k-th run of class c is k = rf[c (d + 1) + j] - rf[c (d + 1)] at its head j
__global__ __launch_bounds__(kRvThreads) void k_tl_runs(uint32_t d, const int64_t *val, const uint32_t *cnt,
                                                        size_t dcap, const uint32_t *rf, uint32_t cap, int64_t *lo,
                                                        int64_t *hi, uint32_t *mult)
{
    const int c = blockIdx.y;
    const uint32_t j = blockIdx.x * kRvThreads + threadIdx.x;
    if (j >= d) return;
    const uint32_t m = tl_mult(c, cnt[j], cnt[dcap + j], cnt[2 * dcap + j]);
    if (!m) return;
    const uint32_t *f = rf + (size_t)c * ((size_t)d + 1);
    const uint32_t base = f[0], k0 = f[j] - base, k1 = f[j + 1] - base;  // k1: heads at or before j
    if (k1 != k0 && k0 < cap) {
        lo[(size_t)c * cap + k0] = val[j];
        mult[(size_t)c * cap + k0] = m;
    }
    const bool tail = !(j + 1 < d && tl_joined(c, val, cnt, dcap, j, m));
    if (tail && k1 - 1 < cap) hi[(size_t)c * cap + k1 - 1] = val[j];
}

// One read per group of G lanes (G a power of two <= 64: a group never spans
// two waves).  flag: [n_reads + 1] the bad reads (0 at n_reads).
template <int G>
__global__ __launch_bounds__(kRvThreads) void k_bank(size_t n_reads, const uint64_t *off, const int64_t *bal,
                                                     uint64_t n, int64_t total, uint8_t *kind, int64_t *found,
                                                     uint32_t *neg, uint32_t *flag, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][kBkN];
    const size_t r = ((size_t)blockIdx.x * kRvThreads + threadIdx.x) / G;
    const uint32_t g = threadIdx.x & (G - 1);
    const bool in = r < n_reads;
    uint64_t b = 0, e = 0, sum = 0;
    uint32_t ng = 0;
    if (in) {
        b = off[r];
        e = off[r + 1];
    }
    for (uint64_t i = b + g; i < e; i += G) {
        const int64_t x = bal[i];
        sum += (uint64_t)x;  // wraps
        ng += x < 0;
    }
#pragma unroll
    for (int o = G >> 1; o > 0; o >>= 1) {
        sum += __shfl_xor((unsigned long long)sum, o, 64);
        ng += __shfl_xor(ng, o, 64);
    }
    uint32_t v[kBkN] = {0, 0, 0, 0};
    if (in && g == 0) {
        const uint64_t len = e - b;
        const uint8_t k = len != n ? 1 : (int64_t)sum != total ? 2 : 0;
        kind[r] = k;
        found[r] = k == 1 ? (int64_t)len : (int64_t)sum;
        neg[r] = ng;
        flag[r] = k != 0;
        v[kBkBad] = k != 0;
        v[kBkWrongN] = k == 1;
        v[kBkWrongTotal] = k == 2;
        v[kBkNegative] = ng != 0;
    } else if (r == n_reads && g == 0) {
        flag[r] = 0;
    }
    block_add<kBkN>(v, ct, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_bank_list(size_t n_reads, const uint32_t *pos, uint32_t cap,
                                                          uint64_t *listed)
{
    const size_t r = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (r >= n_reads) return;
    const uint32_t p = pos[r];
    if (pos[r + 1] == p || p >= cap) return;
    listed[p] = r;
}

}  // namespace

void TallyBufs::release_all()
{
    t.release_all();
    DBuf *all[] = {&in, &rows, &pay, &f0, &f1, &spos, &vsub, &val, &cnt, &rf, &ct, &lo, &hi, &mult};
    for (DBuf *b : all) b->release();
}

void BankBufs::release_all()
{
    DBuf *all[] = {&off, &bal, &kind, &found, &neg, &flag, &scratch, &ct, &listed};
    for (DBuf *b : all) b->release();
}

#define CK(x)                          \
    do {                               \
        hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return e_; \
    } while (0)

hipError_t tally_run(const TallyIn &in, TallyBufs &b, TallyOut &o, hipStream_t s)
{
    constexpr int NC = HSC_TALLY_NCLASS;
    constexpr uint32_t cap = HSC_TALLY_LIST_CAP;
    const size_t n = in.n_attempt + in.n_ack + in.n_seen;
    o = TallyOut{};
    for (int c = 0; c < NC; ++c) {
        o.lo[c].assign(1, 0);
        o.hi[c].assign(1, 0);
        o.mult[c].assign(1, 0);
    }
    if (!n) return hipSuccess;
    ResolveBufs &r = b.t;
    CK(b.in.ensure(8 * n));
    CK(b.rows.ensure(8 * 2 * n));
    CK(b.pay.ensure(8 * n));
    CK(b.f0.ensure(4 * (n + 1)));
    CK(b.f1.ensure(4 * (n + 1)));
    CK(b.spos.ensure(4 * (n + 1)));
    CK(b.vsub.ensure(4 * (n + 1)));
    CK(b.ct.ensure(8 * kTlN));
    CK(b.lo.ensure(8 * (size_t)NC * cap));
    CK(b.hi.ensure(8 * (size_t)NC * cap));
    CK(b.mult.ensure(4 * (size_t)NC * cap));
    // the sort's alternates and scratch (sort_rows2)
    CK(r.words2.ensure(8 * 2 * n));
    CK(r.pay2.ensure(8 * n));
    CK(r.gid.ensure(4 * n));
    CK(r.gid2.ensure(4 * n));
    CK(r.k0.ensure(8 * n));
    CK(r.k1.ensure(8 * n));
    CK(r.words_dev.ensure(256));
    CK(r.scratch.ensure(std::max(std::max(radix_scratch_bytes(n, 2), packed_scratch_bytes(n)),
                                 scan_scratch_bytes((size_t)NC * (n + 1)) + 64)));
    uint64_t *din = b.in.as<uint64_t>(), *rows = b.rows.as<uint64_t>(), *pay = b.pay.as<uint64_t>();
    uint32_t *f0 = b.f0.as<uint32_t>(), *f1 = b.f1.as<uint32_t>(), *spos = b.spos.as<uint32_t>(),
             *vsub = b.vsub.as<uint32_t>();
    unsigned long long *ct = (unsigned long long *)b.ct.p;
    if (in.n_attempt) CK(hipMemcpyAsync(din, in.attempt, 8 * in.n_attempt, hipMemcpyHostToDevice, s));
    if (in.n_ack) CK(hipMemcpyAsync(din + in.n_attempt, in.ack, 8 * in.n_ack, hipMemcpyHostToDevice, s));
    if (in.n_seen)
        CK(hipMemcpyAsync(din + in.n_attempt + in.n_ack, in.seen, 8 * in.n_seen, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(ct, 0, 8 * kTlN, s));
    k_tl_rows<<<tl_blocks(n), kRvThreads, 0, s>>>(n, in.n_attempt, in.n_ack, din, n, rows, pay);
    CK(hipGetLastError());
    const uint64_t *ws, *ps;
    bool pk = false;
    CK(sort_rows2(n, n, r, rows, pay, &pk, &ws, &ps, s));
    o.sort_packed = pk;
    uint32_t *scratch = r.scratch.as<uint32_t>();
    k_tl_heads<<<tl_blocks(n + 1), kRvThreads, 0, s>>>(n, ws, n, f0, f1);
    CK(hipGetLastError());
    CK(scan_exclusive_u32(f0, n + 1, scratch, s));
    CK(scan_exclusive_u32(f1, n + 1, scratch, s));
    k_tl_pos<<<tl_blocks(n + 1), kRvThreads, 0, s>>>(n, f0, f1, spos, vsub);
    CK(hipGetLastError());
    uint32_t d = 0;
    CK(hipMemcpyAsync(&d, f1 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    const size_t dcap = d;  // (n >= 1: d >= 1)
    CK(b.val.ensure(8 * dcap));
    CK(b.cnt.ensure(4 * 3 * dcap));
    CK(b.rf.ensure(4 * (size_t)NC * (dcap + 1)));
    int64_t *val = b.val.as<int64_t>();
    uint32_t *cnt = b.cnt.as<uint32_t>(), *rf = b.rf.as<uint32_t>();
    k_tl_class<<<tl_blocks(d), kRvThreads, 0, s>>>(d, ws, n, spos, vsub, in.multiset ? 1 : 0, dcap, val, cnt, ct);
    CK(hipGetLastError());
    const dim3 grid(tl_blocks((size_t)d + 1), NC);
    k_tl_runflags<<<grid, kRvThreads, 0, s>>>(d, val, cnt, dcap, rf, ct);
    CK(hipGetLastError());
    CK(scan_exclusive_u32(rf, (size_t)NC * (dcap + 1), scratch, s));
    k_tl_runs<<<grid, kRvThreads, 0, s>>>(d, val, cnt, dcap, rf, cap, b.lo.as<int64_t>(), b.hi.as<int64_t>(),
                                          b.mult.as<uint32_t>());
    CK(hipGetLastError());
    unsigned long long hct[kTlN] = {};
    CK(hipMemcpyAsync(hct, ct, 8 * kTlN, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    o.distinct = d;
    for (int k = 0; k < 3; ++k) o.total[k] = hct[kTlTotal + k];
    bool any = false;
    for (int c = 0; c < NC; ++c) {
        o.count[c] = hct[kTlCount + c];
        o.ndistinct[c] = hct[kTlDistinct + c];
        o.runs[c] = hct[kTlRuns + c];
        o.n_listed[c] = (uint32_t)std::min<uint64_t>(o.runs[c], cap);
        if (!o.n_listed[c]) continue;
        const size_t k = o.n_listed[c];
        o.lo[c].resize(k);
        o.hi[c].resize(k);
        o.mult[c].resize(k);
        CK(hipMemcpyAsync(o.lo[c].data(), b.lo.as<int64_t>() + (size_t)c * cap, 8 * k, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.hi[c].data(), b.hi.as<int64_t>() + (size_t)c * cap, 8 * k, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.mult[c].data(), b.mult.as<uint32_t>() + (size_t)c * cap, 4 * k, hipMemcpyDeviceToHost,
                          s));
        any = true;
    }
    if (any) CK(hipStreamSynchronize(s));
    return hipSuccess;
}

template <int G>
static hipError_t bank_launch(const BankIn &in, BankBufs &b, hipStream_t s)
{
    const size_t lanes = (in.n_reads + 1) * (size_t)G;  // (one group past the reads clears the flag there)
    k_bank<G><<<tl_blocks(lanes), kRvThreads, 0, s>>>(in.n_reads, b.off.as<uint64_t>(), b.bal.as<int64_t>(), in.n,
                                                      in.total, b.kind.as<uint8_t>(), b.found.as<int64_t>(),
                                                      b.neg.as<uint32_t>(), b.flag.as<uint32_t>(),
                                                      (unsigned long long *)b.ct.p);
    return hipGetLastError();
}

int bank_group(uint64_t n)
{
    int g = 1;
    while (g < 64 && (uint64_t)g < n) g <<= 1;
    return g;
}

hipError_t bank_run(const BankIn &in, BankBufs &b, BankOut &o, hipStream_t s)
{
    const size_t nr = in.n_reads;
    o = BankOut{};
    o.kind.assign(std::max<size_t>(nr, 1), 0);
    o.found.assign(std::max<size_t>(nr, 1), 0);
    o.neg.assign(std::max<size_t>(nr, 1), 0);
    o.listed.assign(1, 0);
    o.group = bank_group(in.n);
    if (!nr) return hipSuccess;
    const size_t nb = in.off[nr];
    CK(b.off.ensure(8 * (nr + 1)));
    CK(b.bal.ensure(8 * std::max<size_t>(nb, 1)));
    CK(b.kind.ensure(nr));
    CK(b.found.ensure(8 * nr));
    CK(b.neg.ensure(4 * nr));
    CK(b.flag.ensure(4 * (nr + 1)));
    CK(b.scratch.ensure(scan_scratch_bytes(nr + 1) + 64));
    CK(b.ct.ensure(8 * kBkN));
    CK(b.listed.ensure(8 * HSC_BANK_LIST_CAP));
    CK(hipMemcpyAsync(b.off.p, in.off, 8 * (nr + 1), hipMemcpyHostToDevice, s));
    if (nb) CK(hipMemcpyAsync(b.bal.p, in.balance, 8 * nb, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(b.ct.p, 0, 8 * kBkN, s));
    switch (o.group) {
    case 1: CK(bank_launch<1>(in, b, s)); break;
    case 2: CK(bank_launch<2>(in, b, s)); break;
    case 4: CK(bank_launch<4>(in, b, s)); break;
    case 8: CK(bank_launch<8>(in, b, s)); break;
    case 16: CK(bank_launch<16>(in, b, s)); break;
    case 32: CK(bank_launch<32>(in, b, s)); break;
    default: CK(bank_launch<64>(in, b, s)); break;
    }
    unsigned long long hct[kBkN] = {};
    CK(hipMemcpyAsync(hct, b.ct.p, 8 * kBkN, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(o.kind.data(), b.kind.p, nr, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(o.found.data(), b.found.p, 8 * nr, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(o.neg.data(), b.neg.p, 4 * nr, hipMemcpyDeviceToHost, s));
    CK(scan_exclusive_u32(b.flag.as<uint32_t>(), nr + 1, b.scratch.as<uint32_t>(), s));
    k_bank_list<<<tl_blocks(nr), kRvThreads, 0, s>>>(nr, b.flag.as<uint32_t>(), HSC_BANK_LIST_CAP,
                                                     b.listed.as<uint64_t>());
    CK(hipGetLastError());
    CK(hipStreamSynchronize(s));
    o.bad = hct[kBkBad];
    o.wrong_n = hct[kBkWrongN];
    o.wrong_total = hct[kBkWrongTotal];
    o.with_negative = hct[kBkNegative];
    o.n_listed = (uint32_t)std::min<uint64_t>(o.bad, HSC_BANK_LIST_CAP);
    if (o.n_listed) {
        o.listed.resize(o.n_listed);
        CK(hipMemcpyAsync(o.listed.data(), b.listed.p, 8 * (size_t)o.n_listed, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
    }
    return hipSuccess;
}
#undef CK

// load this file's code object now (see warm_graph)
hipError_t warm_tally()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_tl_rows);
}

}  // namespace hsc
