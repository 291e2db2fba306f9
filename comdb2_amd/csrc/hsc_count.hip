// hsc_count.hip -- the reference's checker/counter and checker/queue per
// independent key.  Both are sequential reductions in
// jepsen/checker.clj; here they are sorts, scans and gathers, and every key of
// a call is judged by the same passes.
//
// Passes (the discipline of hsc_tally.hip and hsc_perf.hip: flag + scan
// compaction, so every output is in a defined order; plain stores; the only
// atomics are the key counters, one per workgroup and value that is not zero,
// and the per-key minima):
// counter
//   pair      sort_rows2 (stable) by (key, process, is-info): a process's
//             non-info rows of a key become adjacent in history order.  One
//             kernel over adjacent sorted rows writes invoke_of, the effective
//             value and the row's malformed kind; a second takes the per-key
//             minimum of (op << 3 | kind) over the malformed rows
//   key order (nkeys > 1) one stable sort by key: each key's rows contiguous in
//             history order; the key heads by a search of the sorted keys
//   scans     two scan_exclusive_u64 over the rows' contributions to upper and
//             lower in key order; a key's bound = the prefix minus the prefix
//             at the key's head, exact modulo 2^64
//   reads     the ok reads of well-formed keys flagged, scanned and compacted
//             in (key, j) order, each gathering its invoke's lower; the error
//             flags scanned for the counts and the capped list
// queue, unordered
//             one stable sort by (key, value); +1 / -1 scanned, the prefix at
//             the (key, value) run's head subtracted (heads from a head-flag
//             scan and a compaction); a dequeue whose running count is
//             negative is a candidate, the key's error the candidate of the
//             smallest row
// queue, fifo
//             (nkeys > 1) one stable sort by key; two rank scans (enqueues,
//             dequeues); the enqueue values compacted in key order; the k-th
//             dequeue of a key gathers the key's k-th enqueue
#include <algorithm>

#include "hsc_internal.h"
#include "hsc_table_dev.h"

namespace hsc {

namespace {

constexpr uint64_t kCnSign = 1ull << 63;
constexpr unsigned long long kCnNone = ~0ull;

inline unsigned cn_blocks(size_t n) { return (unsigned)((n + kRvThreads - 1) / kRvThreads); }

// ---- counter ---------------------------------------------------------------
// Row i: ((key, process), is-info), payload i.  key null: key 0
__global__ __launch_bounds__(kRvThreads) void k_cn_rows(size_t n, const uint32_t *key, const uint32_t *proc,
                                                        const uint8_t *type, size_t cap, uint64_t *rows,
                                                        uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= n) return;
    rows[i] = (uint64_t)(key ? key[i] : 0u) << 32 | proc[i];
    rows[cap + i] = type[i] == HSC_OP_INFO;
    pay[i] = i;
}

// Row i: (key, 0), payload i
__global__ __launch_bounds__(kRvThreads) void k_cn_keyrows(size_t n, const uint32_t *key, size_t cap,
                                                           uint64_t *rows, uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= n) return;
    rows[i] = key[i];
    rows[cap + i] = 0;
    pay[i] = i;
}

// ws / ps: the rows sorted by (key, process, is-info) and their ops.  A row
// that is no :info has only such rows before it in its (key, process) group.
__global__ __launch_bounds__(kRvThreads) void k_cn_pair(size_t n, const uint64_t *ws, const uint64_t *ps,
                                                        size_t cap, const uint8_t *type, const uint8_t *f,
                                                        const int64_t *value, int32_t *inv, int64_t *eff,
                                                        uint8_t *malk)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q >= n) return;
    const uint32_t i = (uint32_t)ps[q];
    const uint8_t ty = type[i], fi = f[i];
    const int64_t v = value[i];
    const uint64_t w = ws[q];
    int32_t iv = -1;
    int64_t e = v;
    uint8_t kind = 0;
    if (ty != HSC_OP_INFO) {
        const bool pred = q > 0 && ws[q - 1] == w;
        const uint32_t k = pred ? (uint32_t)ps[q - 1] : 0;
        const bool pred_inv = pred && type[k] == HSC_OP_INVOKE;
        if (ty == HSC_OP_INVOKE) {
            if (q + 1 < n && ws[q + 1] == w && ws[cap + q + 1] == 0) {
                const uint32_t j = (uint32_t)ps[q + 1];
                if (type[j] == HSC_OP_OK) e = value[j];
            }
            if (pred_inv)
                kind = 1;
            else if (fi == HSC_CNT_ADD && e == HSC_CNT_NIL)
                kind = 5;
        } else if (!pred_inv) {
            kind = 2;
        } else {
            iv = (int32_t)k;
            if (ty == HSC_OP_FAIL && v != value[k])
                kind = 3;
            else if (fi != f[k])
                kind = 4;
            else if (ty == HSC_OP_OK && fi != HSC_CNT_OTHER && v == HSC_CNT_NIL)
                kind = 5;
        }
    }
    inv[i] = iv;
    eff[i] = e;
    malk[i] = kind;
}

// kmin[key] = min over the key's malformed rows of (op << 3 | kind)
__global__ __launch_bounds__(kRvThreads) void k_cn_malmin(size_t n, const uint32_t *key, const uint8_t *malk,
                                                          unsigned long long *kmin)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= n) return;
    const uint8_t kind = malk[i];
    if (kind) atomicMin(kmin + (key ? key[i] : 0u), (unsigned long long)i << 3 | kind);
}

// khead[k] (k <= nkeys) = the first sorted position whose key is at least k
// (ws null: one key, khead = {0, n})
__global__ __launch_bounds__(kRvThreads) void k_cn_khead(uint32_t nkeys, size_t n, const uint64_t *ws,
                                                         uint32_t *khead)
{
    const size_t k = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (k > nkeys) return;
    size_t lo = 0, hi = n;
    if (k == nkeys || (!ws && k > 0)) {
        lo = n;
    } else if (ws) {
        while (lo < hi) {
            const size_t mid = lo + ((hi - lo) >> 1);
            if (ws[mid] < k)
                lo = mid + 1;
            else
                hi = mid;
        }
    } else {
        lo = 0;
    }
    khead[k] = (uint32_t)lo;
}

// Position p of the key order holds op ps[p] (ps null: p).  U / L: the row's
// contribution to upper / lower; rflag: an ok read of a well-formed key
// (all [n + 1], 0 at n)
__global__ __launch_bounds__(kRvThreads) void k_cn_contrib(size_t n, const uint64_t *ps, const uint32_t *key,
                                                           const uint8_t *type, const uint8_t *f,
                                                           const int64_t *value, const int64_t *eff,
                                                           const unsigned long long *kmin, uint32_t *ord,
                                                           uint32_t *posof, uint64_t *U, uint64_t *L,
                                                           uint32_t *rflag)
{
    const size_t p = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (p > n) return;
    uint64_t u = 0, l = 0;
    uint32_t r = 0;
    if (p < n) {
        const uint32_t i = ps ? (uint32_t)ps[p] : (uint32_t)p;
        if (ps) {
            ord[p] = i;
            posof[i] = (uint32_t)p;
        }
        const uint8_t ty = type[i], fi = f[i];
        if (fi == HSC_CNT_ADD) {
            if (ty == HSC_OP_INVOKE) u = (uint64_t)eff[i];
            if (ty == HSC_OP_OK) l = (uint64_t)value[i];
        }
        r = ty == HSC_OP_OK && fi == HSC_CNT_READ && kmin[key ? key[i] : 0u] == kCnNone;
    }
    U[p] = u;
    L[p] = l;
    rflag[p] = r;
}

// rpos: rflag scanned; U / L scanned.  Read r of ok read j (invoke i): (lower
// after i, value[j], upper after j) -- neither row contributes to a bound, so
// "after" is the exclusive prefix at its position -- and its error flag
// (eflag[reads] = 0)
__global__ __launch_bounds__(kRvThreads) void k_cn_reads(size_t n, const uint32_t *ord, const uint32_t *posof,
                                                         const uint32_t *key, const int32_t *inv,
                                                         const int64_t *value, const uint64_t *U, const uint64_t *L,
                                                         const uint32_t *rpos, const uint32_t *khead, int64_t *r_lo,
                                                         int64_t *r_val, int64_t *r_hi, uint32_t *r_op,
                                                         uint32_t *eflag)
{
    const size_t p = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (p > n) return;
    const uint32_t r = rpos[p];
    if (p == n) {
        eflag[r] = 0;
        return;
    }
    if (rpos[p + 1] == r) return;
    const uint32_t j = ord ? ord[p] : (uint32_t)p;
    const uint32_t i = (uint32_t)inv[j];  // (a well-formed key: every ok has its invoke)
    const uint32_t pi = posof ? posof[i] : i;
    const uint32_t h = khead[key ? key[j] : 0u];
    const int64_t lo = (int64_t)(L[pi] - L[h]), hi = (int64_t)(U[p] - U[h]), v = value[j];
    r_lo[r] = lo;
    r_val[r] = v;
    r_hi[r] = hi;
    r_op[r] = j;
    eflag[r] = !(lo <= v && v <= hi);
}

// epos: eflag scanned.  The e-th error read (e < cap) is read r
__global__ __launch_bounds__(kRvThreads) void k_cn_list(size_t nr, const uint32_t *epos, uint32_t cap,
                                                        uint32_t *listed)
{
    const size_t r = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (r >= nr) return;
    const uint32_t e = epos[r];
    if (epos[r + 1] != e && e < cap) listed[e] = (uint32_t)r;
}

// Per key (k <= nkeys: read_off has nkeys + 1 entries).  epos null: no reads.
// ct: [0] bad keys, [1] unknown keys
__global__ __launch_bounds__(kRvThreads) void k_cn_keys(uint32_t nkeys, const uint32_t *khead, const uint32_t *rpos,
                                                        const uint32_t *epos, const unsigned long long *kmin,
                                                        uint8_t *verdict, uint32_t *mal_op, uint8_t *mal_kind,
                                                        uint32_t *read_off, uint32_t *errors,
                                                        unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][2];
    const size_t k = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[2] = {0, 0};
    if (k <= nkeys) {
        const uint32_t r0 = rpos[khead[k]];
        read_off[k] = r0;
        if (k < nkeys) {
            const uint32_t r1 = rpos[khead[k + 1]];
            const uint32_t e = epos ? epos[r1] - epos[r0] : 0;
            const unsigned long long m = kmin[k];
            errors[k] = e;
            mal_op[k] = m == kCnNone ? 0xFFFFFFFFu : (uint32_t)(m >> 3);
            mal_kind[k] = m == kCnNone ? 0 : (uint8_t)(m & 7);
            verdict[k] = m != kCnNone ? HSC_CNT_UNKNOWN : e ? HSC_CNT_BAD : HSC_CNT_OK;
            v[0] = m == kCnNone && e;
            v[1] = m != kCnNone;
        }
    }
    block_add<2>(v, ct, lds);
}

// ---- queue -----------------------------------------------------------------
// Row i: (key, value ^ sign bit), payload i
__global__ __launch_bounds__(kRvThreads) void k_q_rows(size_t n, const uint32_t *key, const int64_t *value,
                                                       size_t cap, uint64_t *rows, uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= n) return;
    rows[i] = key ? key[i] : 0u;
    rows[cap + i] = (uint64_t)value[i] ^ kCnSign;
    pay[i] = i;
}

// Unordered: c[q] = +1 / -1 (mod 2^32) of the row at sorted position q, h[q] =
// it heads a (key, value) run (both [n + 1], 0 at n)
__global__ __launch_bounds__(kRvThreads) void k_q_contrib_u(size_t n, const uint64_t *ws, const uint64_t *ps,
                                                            size_t cap, const uint8_t *f, uint32_t *c, uint32_t *h)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > n) return;
    uint32_t cv = 0, hv = 0;
    if (q < n) {
        cv = f[(uint32_t)ps[q]] == HSC_Q_ENQUEUE ? 1u : 0xFFFFFFFFu;
        hv = q == 0 || ws[q] != ws[q - 1] || ws[cap + q] != ws[cap + q - 1];
    }
    c[q] = cv;
    h[q] = hv;
}

// h scanned: rpos[k] = the k-th run's first position (rpos[runs] = n)
__global__ __launch_bounds__(kRvThreads) void k_q_rpos(size_t n, const uint32_t *h, uint32_t *rpos)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > n) return;
    const uint32_t k = h[q];
    if (q == n)
        rpos[k] = (uint32_t)n;
    else if (h[q + 1] != k)
        rpos[k] = (uint32_t)q;
}

// c, h scanned.  A dequeue whose value's running count (this row included) is
// negative: a candidate for its key's error
__global__ __launch_bounds__(kRvThreads) void k_q_cand_u(size_t n, const uint64_t *ws, const uint64_t *ps,
                                                         const uint8_t *f, const uint32_t *c, const uint32_t *h,
                                                         const uint32_t *rpos, unsigned long long *kmin)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q >= n) return;
    const uint32_t i = (uint32_t)ps[q];
    if (f[i] != HSC_Q_DEQUEUE) return;
    const uint32_t head = rpos[h[q + 1] - 1];
    if ((int32_t)(c[q + 1] - c[head]) < 0) atomicMin(kmin + (uint32_t)ws[q], (unsigned long long)i << 3 | 1);
}

// Unordered: ff[q] = position q heads a run of a good key with elements left
// ([n + 1], 0 at n)
__global__ __launch_bounds__(kRvThreads) void k_q_fflag_u(size_t n, const uint64_t *ws, const uint32_t *c,
                                                          const uint32_t *h, const uint32_t *rpos,
                                                          const unsigned long long *kmin, uint32_t *ff)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > n) return;
    uint32_t v = 0;
    if (q < n && h[q + 1] != h[q] && kmin[(uint32_t)ws[q]] == kCnNone)
        v = (int32_t)(c[rpos[h[q] + 1]] - c[q]) > 0;
    ff[q] = v;
}

// ff scanned: the listed runs' values and multiplicities
__global__ __launch_bounds__(kRvThreads) void k_q_final_u(size_t n, const uint64_t *ws, size_t cap,
                                                          const uint32_t *c, const uint32_t *h, const uint32_t *rpos,
                                                          const uint32_t *ff, int64_t *fval, uint32_t *fmult)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q >= n) return;
    const uint32_t p = ff[q];
    if (ff[q + 1] == p) return;
    fval[p] = (int64_t)(ws[cap + q] ^ kCnSign);
    fmult[p] = c[rpos[h[q] + 1]] - c[q];
}

// Unordered: final_off[k] (k <= nkeys) = ff scanned, at the key's head
__global__ __launch_bounds__(kRvThreads) void k_q_off_u(uint32_t nkeys, const uint32_t *khead, const uint32_t *ff,
                                                        uint32_t *off)
{
    const size_t k = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (k > nkeys) return;
    off[k] = ff[khead[k]];
}

// Fifo: e / d [n + 1] = the row at position p of the key order is an enqueue /
// a dequeue (0 at n).  ps null: position p holds row p
__global__ __launch_bounds__(kRvThreads) void k_q_contrib_f(size_t n, const uint64_t *ps, const uint8_t *f,
                                                            uint32_t *e, uint32_t *d)
{
    const size_t p = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (p > n) return;
    uint32_t ev = 0, dv = 0;
    if (p < n) {
        ev = f[ps ? (uint32_t)ps[p] : (uint32_t)p] == HSC_Q_ENQUEUE;
        dv = !ev;
    }
    e[p] = ev;
    d[p] = dv;
}

// e scanned: the enqueue values compacted in key order
__global__ __launch_bounds__(kRvThreads) void k_q_enqval(size_t n, const uint64_t *ps, const int64_t *value,
                                                         const uint32_t *e, int64_t *ev)
{
    const size_t p = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t x = e[p];
    if (e[p + 1] != x) ev[x] = value[ps ? (uint32_t)ps[p] : (uint32_t)p];
}

// e, d scanned.  The k-th dequeue of a key with b enqueues of the key before
// it: empty when b <= k, else a mismatch when the key's k-th enqueue holds
// another value
__global__ __launch_bounds__(kRvThreads) void k_q_cand_f(size_t n, const uint64_t *ps, const uint32_t *key,
                                                         const int64_t *value, const uint32_t *e, const uint32_t *d,
                                                         const uint32_t *khead, const int64_t *ev,
                                                         unsigned long long *kmin)
{
    const size_t p = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (p >= n) return;
    if (d[p + 1] == d[p]) return;
    const uint32_t i = ps ? (uint32_t)ps[p] : (uint32_t)p;
    const uint32_t k = key ? key[i] : 0u;
    const uint32_t h = khead[k];
    const uint32_t kq = d[p] - d[h], b = e[p] - e[h];
    uint32_t kind = 0;
    if (b <= kq)
        kind = 2;
    else if (value[i] != ev[e[h] + kq])  // (e[h] + kq < e[p]: inside ev)
        kind = 1;
    if (kind) atomicMin(kmin + k, (unsigned long long)i << 3 | kind);
}

// Per key (k <= nkeys).  plus / minus scanned ([n + 1]): the key's elements
// left = its plus minus its minus (minus null: none); flen[nkeys] = 0.
// ct: [0] bad keys
__global__ __launch_bounds__(kRvThreads) void k_q_keys(uint32_t nkeys, const uint32_t *khead, const uint32_t *plus,
                                                       const uint32_t *minus, const unsigned long long *kmin,
                                                       uint8_t *verdict, uint32_t *erow, uint8_t *ekind,
                                                       uint32_t *flen, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][1];
    const size_t k = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[1] = {0};
    if (k < nkeys) {
        const uint32_t h0 = khead[k], h1 = khead[k + 1];
        const unsigned long long m = kmin[k];
        const bool bad = m != kCnNone;
        uint32_t len = plus[h1] - plus[h0];
        if (minus) len -= minus[h1] - minus[h0];
        verdict[k] = bad ? HSC_CNT_BAD : HSC_CNT_OK;
        erow[k] = bad ? (uint32_t)(m >> 3) : 0xFFFFFFFFu;
        ekind[k] = bad ? (uint8_t)(m & 7) : 0;
        flen[k] = bad ? 0 : len;
        v[0] = bad;
    } else if (k == nkeys) {
        flen[k] = 0;
    }
    block_add<1>(v, ct, lds);
}

// Fifo: off = flen scanned.  Enqueue number r of a good key that saw dk
// dequeues stays when r >= dk, at off[key] + r - dk
__global__ __launch_bounds__(kRvThreads) void k_q_final_f(size_t n, const uint64_t *ps, const uint32_t *key,
                                                          const int64_t *value, const uint32_t *e, const uint32_t *d,
                                                          const uint32_t *khead, const unsigned long long *kmin,
                                                          const uint32_t *off, int64_t *fval, uint32_t *fmult)
{
    const size_t p = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (p >= n) return;
    if (e[p + 1] == e[p]) return;
    const uint32_t i = ps ? (uint32_t)ps[p] : (uint32_t)p;
    const uint32_t k = key ? key[i] : 0u;
    if (kmin[k] != kCnNone) return;
    const uint32_t h0 = khead[k], h1 = khead[k + 1];
    const uint32_t r = e[p] - e[h0], dk = d[h1] - d[h0];
    if (r < dk) return;
    const uint32_t pos = off[k] + r - dk;  // (below off[k + 1]: r < the key's enqueues)
    fval[pos] = value[i];
    fmult[pos] = 1;
}

}  // namespace

void CountBufs::release_all()
{
    t.release_all();
    DBuf *all[] = {&type, &f, &proc, &value, &key, &rows, &pay, &inv, &eff, &malk, &ord, &posof, &a0, &a1, &s64,
                   &f0, &f1, &f2, &rpos, &khead, &kmin, &ct, &k_verdict, &k_op, &k_kind, &k_u0, &k_off, &r_lo,
                   &r_val, &r_hi, &r_op, &r_list};
    for (DBuf *b : all) b->release();
}

#define CK(x)                          \
    do {                               \
        hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return e_; \
    } while (0)

// A DBuf's first k elements into v (never left empty)
template <class T>
static hipError_t cn_fetch(std::vector<T> &v, const DBuf &b, size_t k, hipStream_t s)
{
    v.assign(std::max<size_t>(k, 1), 0);
    if (!k) return hipSuccess;
    return hipMemcpyAsync(v.data(), b.p, sizeof(T) * k, hipMemcpyDeviceToHost, s);
}

// The sort's alternates and scratch (sort_rows2) for n rows, the scans' scratch
// for n + 1 or nkeys + 1 elements, the per-key buffers both entries share
static hipError_t cn_ensure(CountBufs &b, size_t n, uint32_t nkeys)
{
    ResolveBufs &r = b.t;
    CK(b.rows.ensure(8 * 2 * n));
    CK(b.pay.ensure(8 * n));
    CK(r.words2.ensure(8 * 2 * n));
    CK(r.pay2.ensure(8 * n));
    CK(r.gid.ensure(4 * n));
    CK(r.gid2.ensure(4 * n));
    CK(r.k0.ensure(8 * n));
    CK(r.k1.ensure(8 * n));
    CK(r.words_dev.ensure(256));
    const size_t m = std::max<size_t>(n, nkeys) + 1;
    CK(r.scratch.ensure(std::max(std::max(radix_scratch_bytes(n, 2), packed_scratch_bytes(n)),
                                 scan_scratch_bytes(m) + 64)));
    const size_t nk = (size_t)nkeys + 1;
    CK(b.khead.ensure(4 * nk));
    CK(b.kmin.ensure(8 * nk));
    CK(b.ct.ensure(8 * 2));
    CK(b.k_verdict.ensure(nk));
    CK(b.k_op.ensure(4 * nk));
    CK(b.k_kind.ensure(nk));
    CK(b.k_u0.ensure(4 * nk));
    CK(b.k_off.ensure(4 * nk));
    for (DBuf *x : {&b.f0, &b.f1, &b.f2, &b.rpos}) CK(x->ensure(4 * (n + 2)));
    return hipSuccess;
}

hipError_t counter_run(const CounterIn &in, CountBufs &b, CounterOut &o, hipStream_t s)
{
    constexpr uint32_t cap = HSC_COUNTER_LIST_CAP;
    const size_t n = in.n;
    const uint32_t nkeys = in.nkeys;
    o = CounterOut{};
    o.verdict.assign(nkeys, HSC_CNT_OK);
    o.mal_kind.assign(nkeys, 0);
    o.mal_op.assign(nkeys, 0xFFFFFFFFu);
    o.read_off.assign((size_t)nkeys + 1, 0);
    o.errors.assign(nkeys, 0);
    o.read_op.assign(1, 0);
    o.listed.assign(1, 0);
    for (std::vector<int64_t> *v : {&o.lower, &o.value, &o.upper}) v->assign(1, 0);
    if (!n) return hipSuccess;
    ResolveBufs &r = b.t;
    CK(cn_ensure(b, n, nkeys));
    CK(b.type.ensure(n));
    CK(b.f.ensure(n));
    CK(b.proc.ensure(4 * n));
    CK(b.value.ensure(8 * n));
    if (in.key) CK(b.key.ensure(4 * n));
    CK(b.inv.ensure(4 * n));
    CK(b.eff.ensure(8 * n));
    CK(b.malk.ensure(n));
    if (nkeys > 1) {
        CK(b.ord.ensure(4 * n));
        CK(b.posof.ensure(4 * n));
    }
    CK(b.a0.ensure(8 * (n + 1)));
    CK(b.a1.ensure(8 * (n + 1)));
    CK(b.s64.ensure(scan_scratch_bytes(n + 1, 8)));
    const uint8_t *type = b.type.as<uint8_t>(), *f = b.f.as<uint8_t>();
    const uint32_t *proc = b.proc.as<uint32_t>(), *key = in.key ? b.key.as<uint32_t>() : nullptr;
    const int64_t *value = b.value.as<int64_t>();
    uint64_t *rows = b.rows.as<uint64_t>(), *pay = b.pay.as<uint64_t>();
    int32_t *inv = b.inv.as<int32_t>();
    int64_t *eff = b.eff.as<int64_t>();
    uint8_t *malk = b.malk.as<uint8_t>();
    uint64_t *U = b.a0.as<uint64_t>(), *L = b.a1.as<uint64_t>();
    uint32_t *rflag = b.f0.as<uint32_t>(), *eflag = b.f1.as<uint32_t>(), *khead = b.khead.as<uint32_t>(),
             *scratch = r.scratch.as<uint32_t>();
    unsigned long long *kmin = (unsigned long long *)b.kmin.p, *ct = (unsigned long long *)b.ct.p;
    CK(hipMemcpyAsync(b.type.p, in.type, n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(b.f.p, in.f, n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(b.proc.p, in.process, 4 * n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(b.value.p, in.value, 8 * n, hipMemcpyHostToDevice, s));
    if (in.key) CK(hipMemcpyAsync(b.key.p, in.key, 4 * n, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(kmin, 0xFF, 8 * (size_t)nkeys, s));
    CK(hipMemsetAsync(ct, 0, 8 * 2, s));
    // ---- pair
    k_cn_rows<<<cn_blocks(n), kRvThreads, 0, s>>>(n, key, proc, type, n, rows, pay);
    CK(hipGetLastError());
    const uint64_t *ws, *ps;
    bool pk = false;
    CK(sort_rows2(n, n, r, rows, pay, &pk, &ws, &ps, s));
    o.sort_packed |= pk ? 1 : 0;
    k_cn_pair<<<cn_blocks(n), kRvThreads, 0, s>>>(n, ws, ps, n, type, f, value, inv, eff, malk);
    CK(hipGetLastError());
    k_cn_malmin<<<cn_blocks(n), kRvThreads, 0, s>>>(n, key, malk, kmin);
    CK(hipGetLastError());
    // ---- key order
    ws = ps = nullptr;
    uint32_t *ord = nullptr, *posof = nullptr;
    if (nkeys > 1) {
        k_cn_keyrows<<<cn_blocks(n), kRvThreads, 0, s>>>(n, key, n, rows, pay);
        CK(hipGetLastError());
        CK(sort_rows2(n, n, r, rows, pay, &pk, &ws, &ps, s));
        o.sort_packed |= pk ? 2 : 0;
        ord = b.ord.as<uint32_t>();
        posof = b.posof.as<uint32_t>();
    }
    k_cn_khead<<<cn_blocks((size_t)nkeys + 1), kRvThreads, 0, s>>>(nkeys, n, ws, khead);
    CK(hipGetLastError());
    // ---- scans
    k_cn_contrib<<<cn_blocks(n + 1), kRvThreads, 0, s>>>(n, ps, key, type, f, value, eff, kmin, ord, posof, U, L,
                                                         rflag);
    CK(hipGetLastError());
    CK(scan_exclusive_u64(U, n + 1, b.s64.as<uint64_t>(), s));
    CK(scan_exclusive_u64(L, n + 1, b.s64.as<uint64_t>(), s));
    CK(scan_exclusive_u32(rflag, n + 1, scratch, s));
    uint32_t nr = 0;
    CK(hipMemcpyAsync(&nr, rflag + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    // ---- reads
    uint32_t ne = 0;
    if (nr) {
        CK(b.r_lo.ensure(8 * (size_t)nr));
        CK(b.r_val.ensure(8 * (size_t)nr));
        CK(b.r_hi.ensure(8 * (size_t)nr));
        CK(b.r_op.ensure(4 * (size_t)nr));
        CK(b.r_list.ensure(4 * (size_t)cap));
        k_cn_reads<<<cn_blocks(n + 1), kRvThreads, 0, s>>>(n, ord, posof, key, inv, value, U, L, rflag, khead,
                                                           b.r_lo.as<int64_t>(), b.r_val.as<int64_t>(),
                                                           b.r_hi.as<int64_t>(), b.r_op.as<uint32_t>(), eflag);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(eflag, (size_t)nr + 1, scratch, s));
        CK(hipMemcpyAsync(&ne, eflag + nr, 4, hipMemcpyDeviceToHost, s));
        k_cn_list<<<cn_blocks(nr), kRvThreads, 0, s>>>(nr, eflag, cap, b.r_list.as<uint32_t>());
        CK(hipGetLastError());
    }
    k_cn_keys<<<cn_blocks((size_t)nkeys + 1), kRvThreads, 0, s>>>(
        nkeys, khead, rflag, nr ? eflag : nullptr, kmin, b.k_verdict.as<uint8_t>(), b.k_op.as<uint32_t>(),
        b.k_kind.as<uint8_t>(), b.k_off.as<uint32_t>(), b.k_u0.as<uint32_t>(), ct);
    CK(hipGetLastError());
    unsigned long long hct[2] = {0, 0};
    CK(hipMemcpyAsync(hct, ct, 8 * 2, hipMemcpyDeviceToHost, s));
    CK(cn_fetch(o.verdict, b.k_verdict, nkeys, s));
    CK(cn_fetch(o.mal_op, b.k_op, nkeys, s));
    CK(cn_fetch(o.mal_kind, b.k_kind, nkeys, s));
    CK(cn_fetch(o.read_off, b.k_off, (size_t)nkeys + 1, s));
    CK(cn_fetch(o.errors, b.k_u0, nkeys, s));
    CK(cn_fetch(o.lower, b.r_lo, nr, s));
    CK(cn_fetch(o.value, b.r_val, nr, s));
    CK(cn_fetch(o.upper, b.r_hi, nr, s));
    CK(cn_fetch(o.read_op, b.r_op, nr, s));
    CK(hipStreamSynchronize(s));
    o.reads = nr;
    o.bad_reads = ne;
    o.n_listed = std::min(ne, cap);
    CK(cn_fetch(o.listed, b.r_list, o.n_listed, s));
    CK(hipStreamSynchronize(s));
    o.bad = (uint32_t)hct[0];
    o.unknown = (uint32_t)hct[1];
    return hipSuccess;
}

hipError_t queue_run(const QueueIn &in, CountBufs &b, QueueOut &o, hipStream_t s)
{
    const size_t n = in.n;
    const uint32_t nkeys = in.nkeys;
    o = QueueOut{};
    o.verdict.assign(nkeys, HSC_CNT_OK);
    o.kind.assign(nkeys, 0);
    o.error_row.assign(nkeys, 0xFFFFFFFFu);
    o.final_len.assign(nkeys, 0);
    o.final_off.assign((size_t)nkeys + 1, 0);
    o.final_mult.assign(1, 0);
    o.final_val.assign(1, 0);
    if (!n) return hipSuccess;
    ResolveBufs &r = b.t;
    CK(cn_ensure(b, n, nkeys));
    CK(b.f.ensure(n));
    CK(b.value.ensure(8 * n));
    if (in.key) CK(b.key.ensure(4 * n));
    if (in.fifo) CK(b.a0.ensure(8 * (n + 1)));
    const uint8_t *f = b.f.as<uint8_t>();
    const uint32_t *key = in.key ? b.key.as<uint32_t>() : nullptr;
    const int64_t *value = b.value.as<int64_t>();
    uint64_t *rows = b.rows.as<uint64_t>(), *pay = b.pay.as<uint64_t>();
    uint32_t *f0 = b.f0.as<uint32_t>(), *f1 = b.f1.as<uint32_t>(), *f2 = b.f2.as<uint32_t>(),
             *rpos = b.rpos.as<uint32_t>(), *khead = b.khead.as<uint32_t>(), *koff = b.k_off.as<uint32_t>(),
             *scratch = r.scratch.as<uint32_t>();
    unsigned long long *kmin = (unsigned long long *)b.kmin.p, *ct = (unsigned long long *)b.ct.p;
    CK(hipMemcpyAsync(b.f.p, in.f, n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(b.value.p, in.value, 8 * n, hipMemcpyHostToDevice, s));
    if (in.key) CK(hipMemcpyAsync(b.key.p, in.key, 4 * n, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(kmin, 0xFF, 8 * (size_t)nkeys, s));
    CK(hipMemsetAsync(ct, 0, 8 * 2, s));
    const uint64_t *ws = nullptr, *ps = nullptr;
    bool pk = false;
    uint32_t nfin = 0;
    // the final queues land in r_val / r_op (an enqueue each at the most)
    if (in.final) {
        CK(b.r_val.ensure(8 * n));
        CK(b.r_op.ensure(4 * n));
    }
    int64_t *fval = b.r_val.as<int64_t>();
    uint32_t *fmult = b.r_op.as<uint32_t>();
    if (!in.fifo) {
        k_q_rows<<<cn_blocks(n), kRvThreads, 0, s>>>(n, key, value, n, rows, pay);
        CK(hipGetLastError());
        CK(sort_rows2(n, n, r, rows, pay, &pk, &ws, &ps, s));
        k_cn_khead<<<cn_blocks((size_t)nkeys + 1), kRvThreads, 0, s>>>(nkeys, n, ws, khead);
        CK(hipGetLastError());
        k_q_contrib_u<<<cn_blocks(n + 1), kRvThreads, 0, s>>>(n, ws, ps, n, f, f0, f1);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(f0, n + 1, scratch, s));
        CK(scan_exclusive_u32(f1, n + 1, scratch, s));
        k_q_rpos<<<cn_blocks(n + 1), kRvThreads, 0, s>>>(n, f1, rpos);
        CK(hipGetLastError());
        k_q_cand_u<<<cn_blocks(n), kRvThreads, 0, s>>>(n, ws, ps, f, f0, f1, rpos, kmin);
        CK(hipGetLastError());
        k_q_keys<<<cn_blocks((size_t)nkeys + 1), kRvThreads, 0, s>>>(nkeys, khead, f0, nullptr, kmin,
                                                                     b.k_verdict.as<uint8_t>(),
                                                                     b.k_op.as<uint32_t>(), b.k_kind.as<uint8_t>(),
                                                                     b.k_u0.as<uint32_t>(), ct);
        CK(hipGetLastError());
        if (in.final) {
            k_q_fflag_u<<<cn_blocks(n + 1), kRvThreads, 0, s>>>(n, ws, f0, f1, rpos, kmin, f2);
            CK(hipGetLastError());
            CK(scan_exclusive_u32(f2, n + 1, scratch, s));
            k_q_final_u<<<cn_blocks(n), kRvThreads, 0, s>>>(n, ws, n, f0, f1, rpos, f2, fval, fmult);
            CK(hipGetLastError());
            k_q_off_u<<<cn_blocks((size_t)nkeys + 1), kRvThreads, 0, s>>>(nkeys, khead, f2, koff);
            CK(hipGetLastError());
            CK(hipMemcpyAsync(&nfin, f2 + n, 4, hipMemcpyDeviceToHost, s));
        }
    } else {
        if (nkeys > 1) {
            k_cn_keyrows<<<cn_blocks(n), kRvThreads, 0, s>>>(n, key, n, rows, pay);
            CK(hipGetLastError());
            CK(sort_rows2(n, n, r, rows, pay, &pk, &ws, &ps, s));
        }
        k_cn_khead<<<cn_blocks((size_t)nkeys + 1), kRvThreads, 0, s>>>(nkeys, n, ws, khead);
        CK(hipGetLastError());
        k_q_contrib_f<<<cn_blocks(n + 1), kRvThreads, 0, s>>>(n, ps, f, f0, f1);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(f0, n + 1, scratch, s));
        CK(scan_exclusive_u32(f1, n + 1, scratch, s));
        int64_t *ev = b.a0.as<int64_t>();
        k_q_enqval<<<cn_blocks(n), kRvThreads, 0, s>>>(n, ps, value, f0, ev);
        CK(hipGetLastError());
        k_q_cand_f<<<cn_blocks(n), kRvThreads, 0, s>>>(n, ps, key, value, f0, f1, khead, ev, kmin);
        CK(hipGetLastError());
        k_q_keys<<<cn_blocks((size_t)nkeys + 1), kRvThreads, 0, s>>>(nkeys, khead, f0, f1, kmin,
                                                                     b.k_verdict.as<uint8_t>(),
                                                                     b.k_op.as<uint32_t>(), b.k_kind.as<uint8_t>(),
                                                                     b.k_u0.as<uint32_t>(), ct);
        CK(hipGetLastError());
        if (in.final) {
            CK(hipMemcpyAsync(koff, b.k_u0.p, 4 * ((size_t)nkeys + 1), hipMemcpyDeviceToDevice, s));
            CK(scan_exclusive_u32(koff, (size_t)nkeys + 1, scratch, s));
            k_q_final_f<<<cn_blocks(n), kRvThreads, 0, s>>>(n, ps, key, value, f0, f1, khead, kmin, koff, fval,
                                                            fmult);
            CK(hipGetLastError());
            CK(hipMemcpyAsync(&nfin, koff + nkeys, 4, hipMemcpyDeviceToHost, s));
        }
    }
    o.sort_packed = pk ? 1 : 0;
    unsigned long long hct[2] = {0, 0};
    CK(hipMemcpyAsync(hct, ct, 8 * 2, hipMemcpyDeviceToHost, s));
    CK(cn_fetch(o.verdict, b.k_verdict, nkeys, s));
    CK(cn_fetch(o.error_row, b.k_op, nkeys, s));
    CK(cn_fetch(o.kind, b.k_kind, nkeys, s));
    CK(cn_fetch(o.final_len, b.k_u0, nkeys, s));
    if (in.final) CK(cn_fetch(o.final_off, b.k_off, (size_t)nkeys + 1, s));
    CK(hipStreamSynchronize(s));
    o.bad = (uint32_t)hct[0];
    o.n_final = nfin;
    if (in.final) {
        CK(cn_fetch(o.final_val, b.r_val, nfin, s));
        CK(cn_fetch(o.final_mult, b.r_op, nfin, s));
        CK(hipStreamSynchronize(s));
    }
    return hipSuccess;
}
#undef CK

// load this file's code object now (see warm_graph)
hipError_t warm_count()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_cn_rows);
}

}  // namespace hsc
