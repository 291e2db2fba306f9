// hsc_resolve.hip -- version resolution: which write each read
// of a value history observed, the aborted / intermediate read flags (G1a /
// G1b), which indeterminate txns committed, and the committed part lowered to
// the device-resident ops graph_build takes.
//
// Passes (flag + scan_exclusive_u32 compaction throughout, so every output
// keeps op order; a plain store of 1 wherever one does; the only atomics are
// the sweeps' change word, one per wave that changed something, and the
// counters, one per workgroup and counter that is not zero):
//   check     per op: txn < ntxn, no write of HSC_VAL_INIT, the write flag;
//             per txn: status <= 2, level = 1 for an OK txn
//   gather    the write ops in op order as rows (key, txn | op) and
//             (key, value | op)
//   finality  stable sort by (key, txn): writers gathered in op order stay in
//             program order inside an equal run, so the last row of a run is
//             the txn's final write of the key
//   table     stable sort by (key, value), payload (op, final bit) and txn;
//             equal neighbours are a duplicated written (key, value)
//   directory 2^D buckets over the table's key range (D from the row count):
//             dir[q] = the first row whose key >= kmin + (q << shift), one
//             thread per bucket searching the sorted keys
//   resolve   one thread per read: its key's bucket, then the lower bound of
//             (key, value) inside it (every row of a key lies in one bucket; a
//             history with one hot key degrades to the plain binary search)
//   recovery  sweeps over the reads; level[t] = the sweep that put t into C,
//             plus one (0: outside).  A sweep takes only the readers of an
//             earlier sweep's level, so what a sweep adds does not depend on
//             the order its threads run in, and the number of sweeps is the
//             depth of the longest recovery chain plus the one that finds
//             nothing; four sweeps are queued per host round trip
//   fates     fate, the scan that gives cid, txn_of_cid
//   counts    the reads of C by flag, the per-txn planes, the kept and listed
//             flags; then txn_g1 from the planes
//   lower     the kept ops compacted into (txn, key, is_write, observed);
//             the listed reads compacted up to the cap
#include <algorithm>

#include "hsc_internal.h"
#include "hsc_table_dev.h"

namespace hsc {

namespace {

constexpr uint32_t kRvInitTxn = 0xFFFFFFFFu, kRvNoTxn = 0xFFFFFFFEu;
constexpr uint64_t kRvNoOp = ~0ull;
constexpr int kRvSweepsPerTrip = 4;
constexpr int kRvMaxDirBits = 26;  // the key directory's buckets (256 MiB of u32)
// device words: [0..3] the input's error words, [4..7] a round trip's change
// words; counters (u64) behind them
constexpr int kRvBadTxn = 0, kRvBadInit = 1, kRvBadStatus = 2, kRvDup = 3, kRvChange = 4, kRvWords = 8;
enum { kCtG1a, kCtG1b, kCtDangling, kCtInternal, kCtRecovered, kCtAborted, kCtDropped, kCtG1aTxns, kCtG1bTxns, kCtN };

inline unsigned rv_blocks(size_t n) { return (unsigned)((n + kRvThreads - 1) / kRvThreads); }

__global__ __launch_bounds__(kRvThreads) void k_rv_check(size_t nops, uint32_t ntxn, const uint32_t *txn,
                                                         const uint8_t *isw, const uint64_t *value,
                                                         uint32_t *wflag, uint32_t *words)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i > nops) return;
    if (i == nops) {
        wflag[i] = 0;
        return;
    }
    const bool w = isw[i] != 0;
    wflag[i] = w;
    if (txn[i] >= ntxn) words[kRvBadTxn] = 1;
    if (w && value[i] == HSC_VAL_INIT) words[kRvBadInit] = 1;
}

__global__ __launch_bounds__(kRvThreads) void k_rv_status(uint32_t ntxn, const uint8_t *status, uint32_t *level,
                                                          uint32_t *words)
{
    const uint32_t t = blockIdx.x * kRvThreads + threadIdx.x;
    if (t >= ntxn) return;
    const uint8_t st = status[t];
    level[t] = st == HSC_TXN_OK;
    if (st > HSC_TXN_UNKNOWN) words[kRvBadStatus] = 1;
}

// rows a: (key, txn), rows b: (key, value), both with the op index as payload
__global__ __launch_bounds__(kRvThreads) void k_rv_place(size_t nops, const uint32_t *txn, const uint64_t *key,
                                                         const uint8_t *isw, const uint64_t *value,
                                                         const uint32_t *wpos, size_t cap, uint64_t *a,
                                                         uint64_t *apay, uint64_t *b, uint64_t *bpay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= nops || !isw[i]) return;
    const size_t p = wpos[i];
    const uint64_t k = key[i];
    a[p] = k;
    a[cap + p] = txn[i];
    apay[p] = i;
    b[p] = k;
    b[cap + p] = value[i];
    bpay[p] = i;
}

__global__ __launch_bounds__(kRvThreads) void k_rv_final(size_t nw, const uint64_t *a, size_t cap,
                                                         const uint64_t *apay, uint8_t *fin)
{
    const size_t j = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (j >= nw) return;
    const bool last = j + 1 == nw || a[j + 1] != a[j] || a[cap + j + 1] != a[cap + j];
    fin[apay[j]] = last;
}

__global__ __launch_bounds__(kRvThreads) void k_rv_table(size_t nw, const uint64_t *b, size_t cap,
                                                         const uint64_t *bpay, const uint32_t *txn,
                                                         const uint8_t *fin, uint64_t *tab_op, uint32_t *tab_txn,
                                                         uint32_t *words)
{
    const size_t j = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (j >= nw) return;
    const uint64_t op = bpay[j];
    tab_op[j] = op | (fin[op] ? kRvFin : 0);
    tab_txn[j] = txn[op];
    if (j + 1 < nw && b[j] == b[j + 1] && b[cap + j] == b[cap + j + 1]) words[kRvDup] = 1;
}

__global__ __launch_bounds__(kRvThreads) void k_rv_dir(size_t nw, const uint64_t *tk, int D, uint32_t *dir)
{
    const uint32_t q = blockIdx.x * kRvThreads + threadIdx.x, nb = 1u << D;
    if (q > nb) return;
    const uint64_t kmin = tk[0], span = tk[nw - 1] - kmin;
    const uint64_t off = rv_shl(q, rv_dir_shift(span, D));
    if (q == nb || off > span) {  // past the last key
        dir[q] = (uint32_t)nw;
        return;
    }
    const uint64_t k = kmin + off;
    size_t lo = 0, hi = nw;
    while (lo < hi) {  // the first row whose key >= k
        const size_t mid = lo + ((hi - lo) >> 1);
        if (tk[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    dir[q] = (uint32_t)lo;
}

__global__ __launch_bounds__(kRvThreads) void k_rv_resolve(size_t nops, size_t nw, const uint32_t *txn,
                                                           const uint64_t *key, const uint8_t *isw,
                                                           const uint64_t *value, const uint8_t *status,
                                                           const uint64_t *tk, const uint64_t *tv,
                                                           const uint64_t *tab_op, const uint32_t *tab_txn,
                                                           int D, const uint32_t *dir, uint64_t *obs_op,
                                                           uint32_t *obs_txn, uint8_t *rflag)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= nops) return;
    uint64_t oo = kRvNoOp;
    uint32_t ot = kRvInitTxn;
    uint8_t f = 0;
    const uint64_t v = value[i];
    if (!isw[i] && v != HSC_VAL_INIT) {
        const uint64_t k = key[i];
        const size_t lo = rv_find(nw, tk, tv, D, dir, k, v);
        if (lo < nw) {
            const uint64_t e = tab_op[lo];
            const uint32_t w = tab_txn[lo];
            oo = e & ~kRvFin;
            ot = w;
            if (w == txn[i])
                f = HSC_RD_INTERNAL;
            else
                f = (status[w] == HSC_TXN_ABORTED ? HSC_RD_ABORTED : 0) | (e & kRvFin ? 0 : HSC_RD_INTERMEDIATE);
        } else {
            ot = kRvNoTxn;
            f = HSC_RD_DANGLING;
        }
    }
    obs_op[i] = oo;
    obs_txn[i] = ot;
    rflag[i] = f;
}

// sweep k (from 1): a read of a txn whose level is in [1, k] that observed an
// UNKNOWN writer still at level 0 puts it at level k + 1
__global__ __launch_bounds__(kRvThreads) void k_rv_sweep(size_t nops, const uint32_t *txn, const uint8_t *isw,
                                                         const uint32_t *obs_txn, const uint8_t *rflag,
                                                         const uint8_t *status, uint32_t *level, uint32_t k,
                                                         uint32_t *change)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    bool ch = false;
    if (i < nops && !isw[i]) {
        const uint32_t w = obs_txn[i];
        if (w < kRvNoTxn && !(rflag[i] & HSC_RD_INTERNAL) && status[w] == HSC_TXN_UNKNOWN) {
            const uint32_t lr = level[txn[i]];
            if (lr != 0 && lr <= k && level[w] == 0) {
                level[w] = k + 1;
                ch = true;
            }
        }
    }
    if (__ballot(ch) != 0 && lane_id() == 0) atomicOr(change, 1u);
}

__global__ __launch_bounds__(kRvThreads) void k_rv_fate(uint32_t ntxn, const uint8_t *status, const uint32_t *level,
                                                        uint8_t *fate, uint32_t *inflag, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][3];
    const uint32_t t = blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[3] = {0, 0, 0};
    if (t < ntxn) {
        const uint8_t st = status[t];
        const bool in = level[t] != 0;
        const uint8_t f = st == HSC_TXN_ABORTED ? 1 : st == HSC_TXN_OK ? 0 : in ? 3 : 2;
        fate[t] = f;
        inflag[t] = in;
        v[0] = f == 3;
        v[1] = f == 1;
        v[2] = f == 2;
    } else if (t == ntxn) {
        inflag[t] = 0;
    }
    block_add<3>(v, ct + kCtRecovered, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_rv_cid(uint32_t ntxn, const uint32_t *level, const uint32_t *pos,
                                                       uint32_t *cid, uint32_t *txn_of)
{
    const uint32_t t = blockIdx.x * kRvThreads + threadIdx.x;
    if (t >= ntxn) return;
    if (level[t]) {
        const uint32_t c = pos[t];
        cid[t] = c;
        txn_of[c] = t;
    } else {
        cid[t] = 0xFFFFFFFFu;
    }
}

__global__ __launch_bounds__(kRvThreads) void k_rv_count(size_t nops, const uint32_t *txn, const uint8_t *isw,
                                                         const uint8_t *rflag, const uint32_t *level,
                                                         uint8_t *plane_a, uint8_t *plane_b, uint32_t *kept,
                                                         uint32_t *listed, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][4];
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[4] = {0, 0, 0, 0};
    if (i < nops) {
        const uint32_t r = txn[i];
        const bool in = level[r] != 0, rd = !isw[i];
        const uint8_t f = rd ? rflag[i] : 0;
        kept[i] = in && !(f & (HSC_RD_DANGLING | HSC_RD_ABORTED));
        listed[i] = in && (f & (HSC_RD_ABORTED | HSC_RD_INTERMEDIATE | HSC_RD_DANGLING));
        if (in) {
            v[0] = (f & HSC_RD_ABORTED) != 0;
            v[1] = (f & HSC_RD_INTERMEDIATE) != 0;
            v[2] = (f & HSC_RD_DANGLING) != 0;
            v[3] = (f & HSC_RD_INTERNAL) != 0;
            if (v[0]) plane_a[r] = 1;
            if (v[1]) plane_b[r] = 1;
        }
    } else if (i == nops) {
        kept[i] = 0;
        listed[i] = 0;
    }
    block_add<4>(v, ct + kCtG1a, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_rv_txn_g1(uint32_t ntxn, const uint8_t *plane_a,
                                                          const uint8_t *plane_b, uint8_t *txn_g1,
                                                          unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][2];
    const uint32_t t = blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[2] = {0, 0};
    if (t < ntxn) {
        v[0] = plane_a[t] != 0;
        v[1] = plane_b[t] != 0;
        txn_g1[t] = (uint8_t)(v[0] | v[1] << 1);
    }
    block_add<2>(v, ct + kCtG1aTxns, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_rv_lower(size_t nops, const uint32_t *txn, const uint64_t *key,
                                                         const uint8_t *isw, const uint32_t *obs_txn,
                                                         const uint32_t *cid, const uint32_t *pos, uint32_t *l_txn,
                                                         uint64_t *l_key, uint8_t *l_isw, uint32_t *l_obs)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= nops) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p) return;
    const bool w = isw[i] != 0;
    const uint32_t o = obs_txn[i];
    l_txn[p] = cid[txn[i]];
    l_key[p] = key[i];
    l_isw[p] = w;
    l_obs[p] = (w || o == kRvInitTxn) ? 0xFFFFFFFFu : cid[o];
}

__global__ __launch_bounds__(kRvThreads) void k_rv_list(size_t nops, const uint32_t *pos, const uint64_t *obs_op,
                                                        uint32_t cap, uint64_t *list_op, uint64_t *list_wop)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= nops) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p || p >= cap) return;
    list_op[p] = i;
    list_wop[p] = obs_op[i];
}

}  // namespace

void ResolveBufs::release_all()
{
    DBuf *all[] = {&in_txn, &in_key, &in_isw, &in_val, &in_status, &f0, &f1, &scratch, &words, &words2,
                   &pay, &pay2, &gid, &gid2, &k0, &k1, &fin, &tab_op, &tab_txn, &obs_op, &obs_txn, &rflag,
                   &level, &fate, &cid, &txn_of, &plane, &txn_g1, &words_dev, &dir, &list_op, &list_wop,
                   &l_txn, &l_key, &l_isw, &l_obs};
    for (DBuf *b : all) b->release();
    kept = 0;
    nc = 0;
    valid = false;
}

#define CK(x)                          \
    do {                               \
        hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return e_; \
    } while (0)

// Stable sort of n rows of two words (w[i], w[cap + i]) with the u64 payload:
// as packed single words when the rows' varying bits and a row index fit 64
// bits, by whole rows otherwise.  The sorted rows end in *ws / *ps.
hipError_t sort_rows2(size_t n, size_t cap, ResolveBufs &r, uint64_t *w, uint64_t *pay, bool *ran_packed,
                      const uint64_t **ws, const uint64_t **ps, hipStream_t s)
{
    *ran_packed = false;
    *ws = w;
    *ps = pay;
    if (n <= 1) return hipSuccess;
    uint32_t *gid = r.gid.as<uint32_t>(), *gid2 = r.gid2.as<uint32_t>();
    uint64_t *w2 = r.words2.as<uint64_t>(), *pay2 = r.pay2.as<uint64_t>();
    // the gid slot is carried and never a digit: all zero
    CK(hipMemsetAsync(gid, 0, 4 * n, s));
    uint64_t vary[3] = {0, 0, 0};
    CK(vary_mask_rows(2, n, gid, w, cap, r.scratch.p, vary, s));
    vary[2] = 0;
    PackPlan P;
    if (packed_plan(2, n, vary, &P, true)) {
        uint64_t *lsn_d = nullptr;
        uint32_t *d_count = r.words_dev.as<uint32_t>() + kRvWords + 2 * kCtN;
        CK(packed_sort_dedupe(P, n, gid, w, pay, cap, r.k0.as<uint64_t>(), r.k1.as<uint64_t>(), gid2, w2, pay2, cap,
                              nullptr, nullptr, 0, &lsn_d, d_count, r.scratch.p, r.scratch.bytes, s));
        *ran_packed = true;
        *ws = w2;
        *ps = pay2;
        return hipSuccess;
    }
    bool alt = false;
    CK(radix_sort_known(2, n, gid, w, pay, cap, gid2, w2, pay2, r.scratch.p, r.scratch.bytes, &alt, vary, s));
    if (alt) {
        *ws = w2;
        *ps = pay2;
    }
    return hipSuccess;
}

// The written (key, value) table of a value history (see the passes above):
// finality, the table sorted by (key, value) -- a duplicate sets
// words[kRvDup] -- and its key directory.  wpos: the exclusive scan of the
// write flags; min_scratch: bytes r.scratch keeps for the caller's scans.
hipError_t value_table_build(size_t n, size_t nw, const uint32_t *txn, const uint64_t *key, const uint8_t *isw,
                             const uint64_t *val, const uint32_t *wpos, ResolveBufs &r, int dir_bits,
                             size_t min_scratch, uint32_t *words, ValueTable *vt, hipStream_t s)
{
    const size_t cap = std::max<size_t>(nw, 1);
    const uint64_t *tk = nullptr;
    r.sort_path = 0;
    if (nw) {
        CK(r.words.ensure(8 * 4 * cap));  // rows a, then rows b
        CK(r.words2.ensure(8 * 2 * cap));
        CK(r.pay.ensure(8 * 2 * cap));
        CK(r.pay2.ensure(8 * cap));
        CK(r.gid.ensure(4 * cap));
        CK(r.gid2.ensure(4 * cap));
        CK(r.k0.ensure(8 * cap));
        CK(r.k1.ensure(8 * cap));
        CK(r.tab_op.ensure(8 * cap));
        CK(r.tab_txn.ensure(4 * cap));
        CK(r.scratch.ensure(std::max(std::max(radix_scratch_bytes(nw, 2), packed_scratch_bytes(nw)),
                                     min_scratch)));
        uint64_t *a = r.words.as<uint64_t>(), *b = a + 2 * cap;
        uint64_t *apay = r.pay.as<uint64_t>(), *bpay = apay + cap;
        k_rv_place<<<rv_blocks(n), kRvThreads, 0, s>>>(n, txn, key, isw, val, wpos, cap, a, apay, b, bpay);
        CK(hipGetLastError());
        const uint64_t *ws, *ps;
        bool pk = false;
        CK(sort_rows2(nw, cap, r, a, apay, &pk, &ws, &ps, s));
        r.sort_path |= pk ? 2 : 0;
        k_rv_final<<<rv_blocks(nw), kRvThreads, 0, s>>>(nw, ws, cap, ps, r.fin.as<uint8_t>());
        CK(hipGetLastError());
        CK(sort_rows2(nw, cap, r, b, bpay, &pk, &ws, &ps, s));
        r.sort_path |= pk ? 1 : 0;
        k_rv_table<<<rv_blocks(nw), kRvThreads, 0, s>>>(nw, ws, cap, ps, txn, r.fin.as<uint8_t>(),
                                                        r.tab_op.as<uint64_t>(), r.tab_txn.as<uint32_t>(), words);
        CK(hipGetLastError());
        tk = ws;
        // the key directory: about 8 rows a bucket
        if (dir_bits < 0) {
            dir_bits = 0;
            while (dir_bits < kRvMaxDirBits && ((size_t)8 << dir_bits) < nw) ++dir_bits;
        }
        dir_bits = std::min(dir_bits, kRvMaxDirBits);
        CK(r.dir.ensure(4 * (((size_t)1 << dir_bits) + 1)));
        k_rv_dir<<<rv_blocks(((size_t)1 << dir_bits) + 1), kRvThreads, 0, s>>>(nw, tk, dir_bits, r.dir.as<uint32_t>());
        CK(hipGetLastError());
    }
    vt->nw = nw;
    vt->cap = cap;
    vt->tk = tk;
    vt->tv = tk ? tk + cap : nullptr;
    vt->tab_op = r.tab_op.as<uint64_t>();
    vt->tab_txn = r.tab_txn.as<uint32_t>();
    vt->dir = r.dir.as<uint32_t>();
    vt->dir_bits = std::max(dir_bits, 0);
    return hipSuccess;
}

hipError_t graph_resolve(const ResolveIn &in, ResolveBufs &r, bool arrays, int dir_bits,
                         ResolveOut &o, hipStream_t s)
{
    const size_t n = in.nops;
    const uint32_t nt = in.ntxn;
    r.valid = false;
    r.kept = 0;
    r.nc = 0;
    r.sort_path = 0;
    o = ResolveOut{};
    o.fate.assign(nt, 0);
    o.txn_g1.assign(nt, 0);
    o.cid.assign(nt, 0xFFFFFFFFu);
    const size_t n1 = std::max<size_t>(n, 1), t1 = std::max<size_t>(nt, 1);
    CK(r.in_txn.ensure(4 * n1));
    CK(r.in_key.ensure(8 * n1));
    CK(r.in_isw.ensure(n1));
    CK(r.in_val.ensure(8 * n1));
    CK(r.in_status.ensure(t1));
    CK(r.f0.ensure(4 * (n1 + 1)));
    CK(r.f1.ensure(4 * (std::max(n1, t1) + 1)));
    CK(r.fin.ensure(n1));
    CK(r.obs_op.ensure(8 * n1));
    CK(r.obs_txn.ensure(4 * n1));
    CK(r.rflag.ensure(n1));
    CK(r.level.ensure(4 * t1));
    CK(r.fate.ensure(t1));
    CK(r.cid.ensure(4 * t1));
    CK(r.txn_of.ensure(4 * t1));
    CK(r.plane.ensure(2 * t1));
    CK(r.txn_g1.ensure(t1));
    CK(r.words_dev.ensure(4 * kRvWords + 8 * kCtN + 64));
    CK(r.list_op.ensure(8 * HSC_RESOLVE_LIST_CAP));
    CK(r.list_wop.ensure(8 * HSC_RESOLVE_LIST_CAP));
    CK(r.scratch.ensure(scan_scratch_bytes(std::max(n1, t1) + 1) + 64));
    uint32_t *words = r.words_dev.as<uint32_t>();
    unsigned long long *ct = (unsigned long long *)(words + kRvWords);
    const uint32_t *txn = r.in_txn.as<uint32_t>();
    const uint64_t *key = r.in_key.as<uint64_t>(), *val = r.in_val.as<uint64_t>();
    const uint8_t *isw = r.in_isw.as<uint8_t>(), *status = r.in_status.as<uint8_t>();
    uint32_t *f0 = r.f0.as<uint32_t>(), *f1 = r.f1.as<uint32_t>(), *level = r.level.as<uint32_t>();
    if (n) {
        CK(hipMemcpyAsync(r.in_txn.p, in.txn, 4 * n, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(r.in_key.p, in.key, 8 * n, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(r.in_isw.p, in.is_write, n, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(r.in_val.p, in.value, 8 * n, hipMemcpyHostToDevice, s));
    }
    if (nt) CK(hipMemcpyAsync(r.in_status.p, in.status, nt, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(words, 0, 4 * kRvWords + 8 * kCtN + 8, s));
    // check + the writers' places
    k_rv_check<<<rv_blocks(n + 1), kRvThreads, 0, s>>>(n, nt, txn, isw, val, f0, words);
    CK(hipGetLastError());
    if (nt) {
        k_rv_status<<<rv_blocks(nt), kRvThreads, 0, s>>>(nt, status, level, words);
        CK(hipGetLastError());
    }
    CK(scan_exclusive_u32(f0, n + 1, r.scratch.as<uint32_t>(), s));
    uint32_t hw[kRvWords] = {}, nw32 = 0;
    CK(hipMemcpyAsync(hw, words, 4 * kRvWords, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&nw32, f0 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    o.bad = (hw[kRvBadTxn] ? 1 : 0) | (hw[kRvBadInit] ? 2 : 0) | (hw[kRvBadStatus] ? 4 : 0);
    if (o.bad) return hipErrorInvalidValue;
    const size_t nw = nw32;
    o.writes = nw;
    o.reads = n - nw;
    // finality and the lookup table
    ValueTable vt{};
    CK(value_table_build(n, nw, txn, key, isw, val, f0, r, dir_bits, scan_scratch_bytes(std::max(n1, t1) + 1) + 64,
                         words, &vt, s));
    const size_t cap = vt.cap;
    const uint64_t *tk = vt.tk;
    dir_bits = vt.dir_bits;
    uint64_t *obs_op = r.obs_op.as<uint64_t>();
    uint32_t *obs_txn = r.obs_txn.as<uint32_t>();
    uint8_t *rflag = r.rflag.as<uint8_t>();
    if (n) {
        k_rv_resolve<<<rv_blocks(n), kRvThreads, 0, s>>>(n, nw, txn, key, isw, val, status, tk, tk + cap,
                                                         r.tab_op.as<uint64_t>(), r.tab_txn.as<uint32_t>(),
                                                         std::max(dir_bits, 0), r.dir.as<uint32_t>(), obs_op,
                                                         obs_txn, rflag);
        CK(hipGetLastError());
    }
    // recovery: rounds of kRvSweepsPerTrip sweeps until a round's last sweep changed nothing
    // (the duplicate word comes back with the first round)
    uint32_t sweeps = 0;
    for (;;) {
        if (n)
            for (int q = 0; q < kRvSweepsPerTrip; ++q) {
                k_rv_sweep<<<rv_blocks(n), kRvThreads, 0, s>>>(n, txn, isw, obs_txn, rflag, status, level,
                                                               sweeps + 1 + q, words + kRvChange + q);
                CK(hipGetLastError());
            }
        CK(hipMemcpyAsync(hw, words, 4 * kRvWords, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        if (hw[kRvDup]) {
            o.bad = 8;
            return hipErrorInvalidValue;
        }
        if (!n) break;
        sweeps += kRvSweepsPerTrip;
        if (!hw[kRvChange + kRvSweepsPerTrip - 1]) break;
        CK(hipMemsetAsync(words + kRvChange, 0, 4 * kRvSweepsPerTrip, s));
    }
    o.sweeps = sweeps;
    // fates, cid
    uint8_t *plane = r.plane.as<uint8_t>();
    CK(hipMemsetAsync(plane, 0, 2 * t1, s));
    k_rv_fate<<<rv_blocks((size_t)nt + 1), kRvThreads, 0, s>>>(nt, status, level, r.fate.as<uint8_t>(), f1, ct);
    CK(hipGetLastError());
    CK(scan_exclusive_u32(f1, (size_t)nt + 1, r.scratch.as<uint32_t>(), s));
    uint32_t nc = 0;
    CK(hipMemcpyAsync(&nc, f1 + nt, 4, hipMemcpyDeviceToHost, s));
    if (nt) {
        k_rv_cid<<<rv_blocks(nt), kRvThreads, 0, s>>>(nt, level, f1, r.cid.as<uint32_t>(), r.txn_of.as<uint32_t>());
        CK(hipGetLastError());
    }
    // counts, kept / listed flags, per-txn bits
    k_rv_count<<<rv_blocks(n + 1), kRvThreads, 0, s>>>(n, txn, isw, rflag, level, plane, plane + t1, f0, f1, ct);
    CK(hipGetLastError());
    k_rv_txn_g1<<<rv_blocks(t1), kRvThreads, 0, s>>>(nt, plane, plane + t1, r.txn_g1.as<uint8_t>(), ct);
    CK(hipGetLastError());
    CK(scan_exclusive_u32(f0, n + 1, r.scratch.as<uint32_t>(), s));
    CK(scan_exclusive_u32(f1, n + 1, r.scratch.as<uint32_t>(), s));
    uint32_t kept = 0, nlist = 0;
    unsigned long long hct[kCtN] = {};
    CK(hipMemcpyAsync(&kept, f0 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&nlist, f1 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(hct, ct, 8 * kCtN, hipMemcpyDeviceToHost, s));
    if (n) {
        k_rv_list<<<rv_blocks(n), kRvThreads, 0, s>>>(n, f1, obs_op, HSC_RESOLVE_LIST_CAP,
                                                      r.list_op.as<uint64_t>(), r.list_wop.as<uint64_t>());
        CK(hipGetLastError());
    }
    CK(hipStreamSynchronize(s));
    // the lowered ops (sized by the kept count, so after the sync)
    const size_t k1 = std::max<size_t>(kept, 1);
    CK(r.l_txn.ensure(4 * k1));
    CK(r.l_key.ensure(8 * k1));
    CK(r.l_isw.ensure(k1));
    CK(r.l_obs.ensure(4 * k1));
    if (n) {
        k_rv_lower<<<rv_blocks(n), kRvThreads, 0, s>>>(n, txn, key, isw, obs_txn, r.cid.as<uint32_t>(), f0,
                                                       r.l_txn.as<uint32_t>(), r.l_key.as<uint64_t>(),
                                                       r.l_isw.as<uint8_t>(), r.l_obs.as<uint32_t>());
        CK(hipGetLastError());
    }
    o.kept_ops = kept;
    o.ncommitted = nc;
    o.n_listed = std::min<uint32_t>(nlist, HSC_RESOLVE_LIST_CAP);
    o.g1a_reads = hct[kCtG1a];
    o.g1b_reads = hct[kCtG1b];
    o.dangling_reads = hct[kCtDangling];
    o.internal_reads = hct[kCtInternal];
    o.recovered = (uint32_t)hct[kCtRecovered];
    o.aborted = (uint32_t)hct[kCtAborted];
    o.dropped = (uint32_t)hct[kCtDropped];
    o.g1a_txns = (uint32_t)hct[kCtG1aTxns];
    o.g1b_txns = (uint32_t)hct[kCtG1bTxns];
    o.txn_of_cid.assign(nc, 0);
    o.listed_op.assign(o.n_listed, 0);
    o.listed_wop.assign(o.n_listed, 0);
    if (nt) {
        CK(hipMemcpyAsync(o.fate.data(), r.fate.p, nt, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.cid.data(), r.cid.p, 4 * (size_t)nt, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.txn_g1.data(), r.txn_g1.p, nt, hipMemcpyDeviceToHost, s));
    }
    if (nc) CK(hipMemcpyAsync(o.txn_of_cid.data(), r.txn_of.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
    if (o.n_listed) {
        CK(hipMemcpyAsync(o.listed_op.data(), r.list_op.p, 8 * (size_t)o.n_listed, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.listed_wop.data(), r.list_wop.p, 8 * (size_t)o.n_listed, hipMemcpyDeviceToHost, s));
    }
    if (arrays && n) {
        o.obs_txn.resize(n);
        o.obs_op.resize(n);
        o.rflag.resize(n);
        CK(hipMemcpyAsync(o.obs_txn.data(), obs_txn, 4 * n, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.obs_op.data(), obs_op, 8 * n, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.rflag.data(), rflag, n, hipMemcpyDeviceToHost, s));
    }
    CK(hipStreamSynchronize(s));
    r.kept = kept;
    r.nc = nc;
    r.in_nops = n;
    r.in_ntxn = nt;
    r.valid = true;
    return hipSuccess;
}
#undef CK

// load this file's code object now (see warm_graph)
hipError_t warm_resolve()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_rv_check);
}

}  // namespace hsc
