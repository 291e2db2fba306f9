// hsc_lists.hip -- list-append histories: every write appends
// a unique element to its key's list and every read returns the whole list, so
// the longest read of a key -- its spine -- is that key's version order.  This
// file recovers the spines, flags the reads against them, decides which
// indeterminate txns committed, and emits the ww / wr / rw edge rows in cid
// space for a graph_build through GraphInput::x_rows.  Nothing is assumed
// about txn ids.
//
// Passes (the discipline of hsc_resolve.hip: flag + scan_exclusive_u32
// compaction, so every output keeps op order; a plain store of 1 wherever one
// does; one atomic per workgroup and counter that is not zero -- and the first
// occurrence's atomic minimum, one per resolved spine element):
//   check     per op: txn < ntxn, list_off ascending, the write flag, the
//             flag of a read by an OK txn; per txn: status <= 2, level = OK
//   reads     the OK reads as rows (key, 2^32 - 1 - length) with the op as
//             payload, gathered in op order and sorted stably: the head of a
//             key's run is its spine (ties: the lowest op), head flags + scan
//             give every read its key rank; the spines' lengths scanned give
//             each its base in the concatenated spine
//   table     the appends sorted by (key, element) with the finality bit and
//             the key directory (value_table_build, shared with the resolve
//             entry); equal neighbours are a duplicated append
//   spine     one thread per spine element: its table row, the atomic minimum
//             of the position per row (the first occurrence), level = 1 for an
//             UNKNOWN writer (recovered: only OK txns read, so one pass)
//   sflags    per spine position: dangling, duplicate, aborted, chain member;
//             four exclusive scans
//   compare   one thread per element of the history: an element of an OK read
//             that is not its key's spine against the spine at the same
//             offset -- the only pass over all the elements, a streaming
//             compare
//   chain     the chain members compacted (writer, key rank); a ww row per
//             neighbouring pair of one key with different writers
//   fates     fate, the scan that gives cid, txn_of_cid
//   reads     per OK read: the flags from the scans at base and base + n, the
//             wr and rw rows from the chain entries around its c members
//   counts    the per-txn planes, unobserved appends per table row,
//             incompatible keys, the listed reads compacted up to the cap
// The edge rows: slots 2 j, 2 j + 1 for the wr / rw row of the j-th OK read,
// then one ww slot per spine position (chain entry x in slot x); a slot
// without an edge holds ~0, which the build's sort drops.
#include <algorithm>

#include "hsc_internal.h"
#include "hsc_table_dev.h"

namespace hsc {

namespace {

constexpr uint32_t kLsNone = 0xFFFFFFFFu;
constexpr int kLsBadTxn = 0, kLsBadOff = 1, kLsBadStatus = 2, kLsDup = 3, kLsWords = 8;
enum {
    kLcG1a, kLcG1b, kLcDangling, kLcDupRd, kLcIncompat, kLcInternal, kLcWr, kLcRw,  // the read pass's eight
    kLcWw, kLcRecovered, kLcAborted, kLcDropped, kLcG1aTxns, kLcG1bTxns, kLcIncKeys, kLcUnobs, kLcN
};
constexpr uint8_t kLsListed =
    HSC_RD_ABORTED | HSC_RD_INTERMEDIATE | HSC_RD_DANGLING | HSC_LRD_DUPLICATE | HSC_LRD_INCOMPATIBLE;

inline unsigned ls_blocks(size_t n) { return (unsigned)((n + kRvThreads - 1) / kRvThreads); }

__global__ __launch_bounds__(kRvThreads) void k_ls_check(size_t nops, uint32_t ntxn, const uint32_t *txn,
                                                         const uint8_t *isw, const uint64_t *off,
                                                         const uint8_t *status, uint32_t *wflag, uint32_t *rdflag,
                                                         uint32_t *words)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i > nops) return;
    if (i == nops) {
        wflag[i] = 0;
        rdflag[i] = 0;
        return;
    }
    const bool w = isw[i] != 0;
    const uint32_t t = txn[i];
    wflag[i] = w;
    rdflag[i] = !w && t < ntxn && status[t] == HSC_TXN_OK;
    if (t >= ntxn) words[kLsBadTxn] = 1;
    if (off[i + 1] < off[i]) words[kLsBadOff] = 1;
}

__global__ __launch_bounds__(kRvThreads) void k_ls_status(uint32_t ntxn, const uint8_t *status, uint32_t *level,
                                                          uint32_t *words)
{
    const uint32_t t = blockIdx.x * kRvThreads + threadIdx.x;
    if (t >= ntxn) return;
    const uint8_t st = status[t];
    level[t] = st == HSC_TXN_OK;
    if (st > HSC_TXN_UNKNOWN) words[kLsBadStatus] = 1;
}

// the OK reads as rows (key, 2^32 - 1 - length), payload the op
__global__ __launch_bounds__(kRvThreads) void k_ls_rd_place(size_t nops, const uint64_t *key, const uint64_t *off,
                                                            const uint32_t *rpos, size_t cap, uint64_t *rows,
                                                            uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= nops) return;
    const uint32_t p = rpos[i];
    if (rpos[i + 1] == p) return;
    rows[p] = key[i];
    rows[cap + p] = 0xFFFFFFFFull - (off[i + 1] - off[i]);
    pay[p] = i;
}

// head[j] = the sorted read j opens a key other than the first
__global__ __launch_bounds__(kRvThreads) void k_ls_heads(size_t nr, const uint64_t *sk, uint32_t *head)
{
    const size_t j = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (j > nr) return;
    head[j] = j > 0 && j < nr && sk[j] != sk[j - 1];
}

// hs: the exclusive scan of the heads, so hs[j + 1] is read j's key rank
__global__ __launch_bounds__(kRvThreads) void k_ls_keys(size_t nr, const uint64_t *sk, size_t cap,
                                                        const uint64_t *sp, const uint32_t *hs, uint32_t *rk,
                                                        uint64_t *sp_op, uint32_t *sp_len, uint32_t *sp_base)
{
    const size_t j = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (j >= nr) return;
    const uint32_t q = hs[j + 1];
    const uint64_t op = sp[j];
    rk[op] = q;
    if (j == 0 || hs[j] != q) {
        const uint32_t len = (uint32_t)(0xFFFFFFFFull - sk[cap + j]);
        sp_op[q] = op;
        sp_len[q] = len;
        sp_base[q] = len;  // (scanned in place)
    }
}

// the key rank whose spine holds position p: the last q with base[q] <= p
__device__ __forceinline__ uint32_t ls_key_of(const uint32_t *base, uint32_t nk, uint32_t p)
{
    uint32_t lo = 0, hi = nk;  // the first q with base[q] > p
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (base[mid] <= p)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;  // (base[0] == 0 <= p)
}

__global__ __launch_bounds__(kRvThreads) void k_ls_spine(uint32_t S, uint32_t nk, const uint32_t *sp_base,
                                                         const uint64_t *sp_op, const uint64_t *key,
                                                         const uint64_t *off, const uint64_t *elems, size_t nw,
                                                         const uint64_t *tk, const uint64_t *tv,
                                                         const uint32_t *tab_txn, int D, const uint32_t *dir,
                                                         const uint8_t *status, uint32_t *s_row, uint32_t *s_q,
                                                         uint32_t *first, uint32_t *level)
{
    const uint32_t p = blockIdx.x * kRvThreads + threadIdx.x;
    if (p >= S) return;
    const uint32_t q = ls_key_of(sp_base, nk, p);
    const uint64_t op = sp_op[q];
    const uint64_t e = elems[off[op] + (p - sp_base[q])];
    const size_t row = rv_find(nw, tk, tv, D, dir, key[op], e);
    s_q[p] = q;
    if (row < nw) {
        s_row[p] = (uint32_t)row;
        atomicMin(first + row, p);
        const uint32_t w = tab_txn[row];
        if (status[w] == HSC_TXN_UNKNOWN) level[w] = 1;
    } else {
        s_row[p] = kLsNone;
    }
}

// the four flag planes of S + 1 words each: dangling, duplicate, aborted, chain
__global__ __launch_bounds__(kRvThreads) void k_ls_sflags(uint32_t S, const uint32_t *s_row, const uint32_t *first,
                                                          const uint32_t *tab_txn, const uint8_t *status,
                                                          const uint32_t *level, uint32_t *pl)
{
    const uint32_t p = blockIdx.x * kRvThreads + threadIdx.x;
    if (p > S) return;
    uint32_t dang = 0, dup = 0, abo = 0, ch = 0;
    if (p < S) {
        const uint32_t row = s_row[p];
        if (row == kLsNone) {
            dang = 1;
        } else {
            const uint32_t w = tab_txn[row];
            dup = first[row] != p;
            abo = status[w] == HSC_TXN_ABORTED;
            ch = !dup && level[w] != 0;
        }
    }
    const size_t st = (size_t)S + 1;
    pl[p] = dang;
    pl[st + p] = dup;
    pl[2 * st + p] = abo;
    pl[3 * st + p] = ch;
}

__global__ __launch_bounds__(kRvThreads) void k_ls_compare(uint64_t E, size_t nops, const uint64_t *off,
                                                           const uint64_t *elems, const uint32_t *rk,
                                                           const uint64_t *sp_op, const uint32_t *sp_len,
                                                           uint8_t *incompat)
{
    const uint64_t g = (uint64_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (g >= E) return;
    size_t lo = 0, hi = nops;  // the first op whose run starts after g
    while (lo < hi) {
        const size_t mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= g)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo == 0) return;  // before the first run
    const size_t i = lo - 1;
    const uint32_t q = rk[i];
    if (q == kLsNone) return;  // not a read of an OK txn
    const uint64_t sop = sp_op[q];
    if (sop == i) return;  // the spine itself
    const uint64_t d = g - off[i];
    if (d >= sp_len[q] || elems[g] != elems[off[sop] + d]) incompat[i] = 1;
}

__global__ __launch_bounds__(kRvThreads) void k_ls_chain(uint32_t S, const uint32_t *sc, const uint32_t *s_row,
                                                         const uint32_t *s_q, const uint32_t *tab_txn,
                                                         uint32_t *chain_w, uint32_t *chain_q)
{
    const uint32_t p = blockIdx.x * kRvThreads + threadIdx.x;
    if (p >= S) return;
    const uint32_t x = sc[p];
    if (sc[p + 1] == x) return;
    chain_w[x] = tab_txn[s_row[p]];
    chain_q[x] = s_q[p];
}

__global__ __launch_bounds__(kRvThreads) void k_ls_fate(uint32_t ntxn, const uint8_t *status, const uint32_t *level,
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
    block_add<3>(v, ct + kLcRecovered, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_ls_cid(uint32_t ntxn, const uint32_t *level, const uint32_t *pos,
                                                       uint32_t *cid, uint32_t *txn_of)
{
    const uint32_t t = blockIdx.x * kRvThreads + threadIdx.x;
    if (t >= ntxn) return;
    if (level[t]) {
        const uint32_t c = pos[t];
        cid[t] = c;
        txn_of[c] = t;
    } else {
        cid[t] = kLsNone;
    }
}

// the ww slots: one per spine position, chain entry x in slot x
__global__ __launch_bounds__(kRvThreads) void k_ls_ww(uint32_t S, const uint32_t *sc, const uint32_t *chain_w,
                                                      const uint32_t *chain_q, const uint32_t *cid, uint64_t *rows,
                                                      uint64_t *type, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][1];
    const uint32_t x = blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[1] = {0};
    if (x < S) {
        const uint32_t nch = sc[S];
        uint64_t row = ~0ull;
        if (x + 1 < nch && chain_q[x] == chain_q[x + 1]) {
            const uint32_t a = chain_w[x], b = chain_w[x + 1];
            if (a != b) {
                row = ((uint64_t)cid[a] << 32) | cid[b];
                v[0] = 1;
            }
        }
        rows[x] = row;
        type[x] = kDepWW;
    }
    block_add<1>(v, ct + kLcWw, lds);
}

// pl: the scanned planes of k_ls_sflags (sd, su, sa, sc)
__global__ __launch_bounds__(kRvThreads) void k_ls_reads(
    size_t nops, uint32_t S, const uint32_t *txn, const uint64_t *off, const uint32_t *rk, const uint32_t *rpos,
    const uint8_t *incompat, const uint32_t *sp_base, const uint32_t *pl, const uint32_t *s_row,
    const uint64_t *tab_op, const uint32_t *tab_txn, const uint32_t *chain_w, const uint32_t *cid, uint8_t *rflag,
    uint8_t *inck, uint8_t *plane_a, uint8_t *plane_b, uint32_t *listed, uint64_t *rows, uint64_t *type,
    unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][8];
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (i < nops) {
        const uint32_t q = rk[i];
        uint8_t f = 0;
        if (q != kLsNone) {
            const uint32_t r = txn[i];
            uint64_t wr = ~0ull, rw = ~0ull;
            if (incompat[i]) {
                f = HSC_LRD_INCOMPATIBLE;
                inck[q] = 1;
                v[kLcIncompat] = 1;
            } else {
                const size_t st = (size_t)S + 1;
                const uint32_t *sd = pl, *su = pl + st, *sa = pl + 2 * st, *sc = pl + 3 * st;
                const uint32_t n = (uint32_t)(off[i + 1] - off[i]);
                const uint32_t b = sp_base[q], e = b + n;
                if (sd[e] != sd[b]) f |= HSC_RD_DANGLING;
                if (su[e] != su[b]) f |= HSC_LRD_DUPLICATE;
                if (sa[e] != sa[b]) f |= HSC_RD_ABORTED;
                if (n) {
                    const uint32_t row = s_row[e - 1];
                    if (row != kLsNone && tab_txn[row] != r && !(tab_op[row] & kRvFin)) f |= HSC_RD_INTERMEDIATE;
                }
                const uint32_t c0 = sc[b], c1 = sc[e], cend = sc[sp_base[q + 1]];
                if (c1 > c0) {  // the last chain member inside the read
                    const uint32_t w = chain_w[c1 - 1];
                    if (w == r)
                        f |= HSC_RD_INTERNAL;
                    else
                        wr = ((uint64_t)cid[w] << 32) | cid[r];
                }
                if (c1 < cend) {  // the first one past it
                    const uint32_t w = chain_w[c1];
                    if (w != r) rw = ((uint64_t)cid[r] << 32) | cid[w];
                }
                v[kLcG1a] = (f & HSC_RD_ABORTED) != 0;
                v[kLcG1b] = (f & HSC_RD_INTERMEDIATE) != 0;
                v[kLcDangling] = (f & HSC_RD_DANGLING) != 0;
                v[kLcDupRd] = (f & HSC_LRD_DUPLICATE) != 0;
                v[kLcInternal] = (f & HSC_RD_INTERNAL) != 0;
                v[kLcWr] = wr != ~0ull;
                v[kLcRw] = rw != ~0ull;
                if (v[kLcG1a]) plane_a[r] = 1;
                if (v[kLcG1b]) plane_b[r] = 1;
            }
            const size_t slot = 2 * (size_t)rpos[i];
            rows[slot] = wr;
            rows[slot + 1] = rw;
            type[slot] = kDepWR;
            type[slot + 1] = kDepRW;
        }
        rflag[i] = f;
        listed[i] = (f & kLsListed) != 0;
    } else if (i == nops) {
        listed[i] = 0;
    }
    block_add<8>(v, ct + kLcG1a, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_ls_txn_g1(uint32_t ntxn, const uint8_t *plane_a,
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
    block_add<2>(v, ct + kLcG1aTxns, lds);
}

// keys with an incompatible read
__global__ __launch_bounds__(kRvThreads) void k_ls_inck(uint32_t nk, const uint8_t *inck, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][1];
    const uint32_t q = blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[1] = {q < nk && inck[q] != 0};
    block_add<1>(v, ct + kLcIncKeys, lds);
}

// appends of txns in C whose element stands in no spine
__global__ __launch_bounds__(kRvThreads) void k_ls_unobs(size_t nw, const uint32_t *tab_txn, const uint32_t *first,
                                                         const uint32_t *level, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][1];
    const size_t j = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[1] = {j < nw && first[j] == kLsNone && level[tab_txn[j]] != 0};
    block_add<1>(v, ct + kLcUnobs, lds);
}

__global__ __launch_bounds__(kRvThreads) void k_ls_list(size_t nops, const uint32_t *pos, const uint8_t *rflag,
                                                        uint32_t cap, uint64_t *list_op, uint8_t *list_flag)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= nops) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p || p >= cap) return;
    list_op[p] = i;
    list_flag[p] = rflag[i];
}

}  // namespace

void ListBufs::release_all()
{
    DBuf *all[] = {&in_txn, &in_key, &in_isw, &in_val, &in_off, &in_elems, &in_status, &f0, &f1, &f2, &f3,
                   &rd_rows, &rd_pay, &rk, &incompat, &rflag, &sp_op, &sp_len, &sp_base, &inck, &s_row, &first,
                   &chain_w, &chain_q, &level, &fate, &cid, &txn_of, &plane, &txn_g1, &words_dev, &list_op,
                   &list_flag, &x_rows, &x_type};
    for (DBuf *b : all) b->release();
    t.release_all();
    n_rows = 0;
    nc = 0;
    valid = false;
}

#define CK(x)                          \
    do {                               \
        hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return e_; \
    } while (0)

hipError_t graph_resolve_lists(const ListIn &in, ListBufs &l, bool arrays, ListOut &o, hipStream_t s)
{
    const size_t n = in.nops;
    const uint32_t nt = in.ntxn;
    const uint64_t E = n ? in.list_off[n] : 0;
    l.valid = false;
    l.n_rows = 0;
    l.nc = 0;
    o = ListOut{};
    o.fate.assign(nt, 0);
    o.txn_g1.assign(nt, 0);
    o.cid.assign(nt, kLsNone);
    const size_t n1 = std::max<size_t>(n, 1), t1 = std::max<size_t>(nt, 1), e1 = std::max<size_t>(E, 1);
    ResolveBufs &tb = l.t;
    CK(l.in_txn.ensure(4 * n1));
    CK(l.in_key.ensure(8 * n1));
    CK(l.in_isw.ensure(n1));
    CK(l.in_val.ensure(8 * n1));
    CK(l.in_off.ensure(8 * (n1 + 1)));
    CK(l.in_elems.ensure(8 * e1));
    CK(l.in_status.ensure(t1));
    CK(l.f0.ensure(4 * (n1 + 1)));
    CK(l.f1.ensure(4 * (n1 + 1)));
    CK(l.rk.ensure(4 * n1));
    CK(l.incompat.ensure(n1));
    CK(l.rflag.ensure(n1));
    CK(l.level.ensure(4 * t1));
    CK(l.fate.ensure(t1));
    CK(l.cid.ensure(4 * t1));
    CK(l.txn_of.ensure(4 * t1));
    CK(l.plane.ensure(2 * t1));
    CK(l.txn_g1.ensure(t1));
    CK(l.words_dev.ensure(4 * kLsWords + 8 * kLcN + 64));
    CK(l.list_op.ensure(8 * HSC_RESOLVE_LIST_CAP));
    CK(l.list_flag.ensure(HSC_RESOLVE_LIST_CAP));
    CK(tb.fin.ensure(n1));
    CK(tb.words_dev.ensure(256));
    CK(tb.scratch.ensure(scan_scratch_bytes(std::max(n1, t1) + 2) + 64));
    uint32_t *words = l.words_dev.as<uint32_t>();
    unsigned long long *ct = (unsigned long long *)(words + kLsWords);
    const uint32_t *txn = l.in_txn.as<uint32_t>();
    const uint64_t *key = l.in_key.as<uint64_t>(), *val = l.in_val.as<uint64_t>();
    const uint64_t *off = l.in_off.as<uint64_t>(), *elems = l.in_elems.as<uint64_t>();
    const uint8_t *isw = l.in_isw.as<uint8_t>(), *status = l.in_status.as<uint8_t>();
    uint32_t *f0 = l.f0.as<uint32_t>(), *f1 = l.f1.as<uint32_t>(), *level = l.level.as<uint32_t>();
    if (n) {
        CK(hipMemcpyAsync(l.in_txn.p, in.txn, 4 * n, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(l.in_key.p, in.key, 8 * n, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(l.in_isw.p, in.is_write, n, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(l.in_val.p, in.value, 8 * n, hipMemcpyHostToDevice, s));
        CK(hipMemcpyAsync(l.in_off.p, in.list_off, 8 * (n + 1), hipMemcpyHostToDevice, s));
    } else {
        CK(hipMemsetAsync(l.in_off.p, 0, 16, s));
    }
    if (E) CK(hipMemcpyAsync(l.in_elems.p, in.elems, 8 * E, hipMemcpyHostToDevice, s));
    if (nt) CK(hipMemcpyAsync(l.in_status.p, in.status, nt, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(words, 0, 4 * kLsWords + 8 * kLcN + 8, s));
    CK(hipMemsetAsync(tb.words_dev.p, 0, 256, s));
    // check, the appends' and the OK reads' places
    k_ls_check<<<ls_blocks(n + 1), kRvThreads, 0, s>>>(n, nt, txn, isw, off, status, f0, f1, words);
    CK(hipGetLastError());
    if (nt) {
        k_ls_status<<<ls_blocks(nt), kRvThreads, 0, s>>>(nt, status, level, words);
        CK(hipGetLastError());
    }
    CK(scan_exclusive_u32(f0, n + 1, tb.scratch.as<uint32_t>(), s));
    CK(scan_exclusive_u32(f1, n + 1, tb.scratch.as<uint32_t>(), s));
    uint32_t hw[kLsWords] = {}, nw32 = 0, nr32 = 0;
    CK(hipMemcpyAsync(hw, words, 4 * kLsWords, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&nw32, f0 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&nr32, f1 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    o.bad = (hw[kLsBadTxn] ? 1 : 0) | (hw[kLsBadOff] ? 2 : 0) | (hw[kLsBadStatus] ? 4 : 0);
    if (o.bad) return hipErrorInvalidValue;
    const size_t nw = nw32, nr = nr32;
    o.appends = nw;
    o.reads = n - nw;
    o.elements = E;
    // the reads sorted by (key, longest first, op): spines and key ranks.  The
    // sort's rows are the table's too, so the reads go first.
    const size_t capm = std::max<size_t>(std::max(nw, nr), 1), capr = std::max<size_t>(nr, 1);
    CK(tb.words2.ensure(8 * 2 * capm));
    CK(tb.pay2.ensure(8 * capm));
    CK(tb.gid.ensure(4 * capm));
    CK(tb.gid2.ensure(4 * capm));
    CK(tb.k0.ensure(8 * capm));
    CK(tb.k1.ensure(8 * capm));
    CK(tb.scratch.ensure(std::max(std::max(radix_scratch_bytes(capm, 2), packed_scratch_bytes(capm)),
                                  scan_scratch_bytes(std::max(n1, t1) + 2) + 64)));
    CK(l.rd_rows.ensure(8 * 2 * capr));
    CK(l.rd_pay.ensure(8 * capr));
    CK(l.f2.ensure(4 * (std::max(capr, t1) + 2)));
    CK(l.sp_op.ensure(8 * (capr + 1)));
    CK(l.sp_len.ensure(4 * (capr + 1)));
    CK(l.sp_base.ensure(4 * (capr + 1)));
    CK(l.inck.ensure(capr + 1));
    uint32_t *f2 = l.f2.as<uint32_t>(), *rk = l.rk.as<uint32_t>();
    uint32_t *sp_len = l.sp_len.as<uint32_t>(), *sp_base = l.sp_base.as<uint32_t>();
    uint64_t *sp_op = l.sp_op.as<uint64_t>();
    CK(hipMemsetAsync(rk, 0xFF, 4 * n1, s));
    CK(hipMemsetAsync(sp_base, 0, 4 * (capr + 1), s));
    CK(hipMemsetAsync(l.incompat.p, 0, n1, s));
    CK(hipMemsetAsync(l.inck.p, 0, capr + 1, s));
    uint32_t nk = 0, S = 0;
    if (nr) {
        uint64_t *rows = l.rd_rows.as<uint64_t>(), *pay = l.rd_pay.as<uint64_t>();
        k_ls_rd_place<<<ls_blocks(n), kRvThreads, 0, s>>>(n, key, off, f1, capr, rows, pay);
        CK(hipGetLastError());
        const uint64_t *ws, *ps;
        bool pk = false;
        CK(sort_rows2(nr, capr, tb, rows, pay, &pk, &ws, &ps, s));
        k_ls_heads<<<ls_blocks(nr + 1), kRvThreads, 0, s>>>(nr, ws, f2);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(f2, nr + 1, tb.scratch.as<uint32_t>(), s));
        k_ls_keys<<<ls_blocks(nr), kRvThreads, 0, s>>>(nr, ws, capr, ps, f2, rk, sp_op, sp_len, sp_base);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(sp_base, nr + 1, tb.scratch.as<uint32_t>(), s));
        CK(hipMemcpyAsync(&nk, f2 + nr, 4, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(&S, sp_base + nr, 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        nk += 1;
    }
    o.keys = nk;
    o.spine_elements = S;
    // the append table (after the reads' sort: it may end in the sort's rows)
    const size_t s1 = std::max<size_t>(S, 1), w1 = std::max<size_t>(nw, 1);
    const size_t scan_need = scan_scratch_bytes(std::max(std::max(n1, t1), s1) + 2) + 64;
    CK(tb.scratch.ensure(scan_need));
    ValueTable vt{};
    CK(value_table_build(n, nw, txn, key, isw, val, f0, tb, -1, scan_need, tb.words_dev.as<uint32_t>(), &vt, s));
    // the spine against the table
    CK(l.s_row.ensure(4 * 2 * s1));
    CK(l.first.ensure(4 * w1));
    CK(l.f3.ensure(4 * 4 * (s1 + 1)));
    CK(l.chain_w.ensure(4 * s1));
    CK(l.chain_q.ensure(4 * s1));
    const size_t n_rows = 2 * nr + S;
    CK(l.x_rows.ensure(8 * std::max<size_t>(n_rows, 1)));
    CK(l.x_type.ensure(8 * std::max<size_t>(n_rows, 1)));
    uint32_t *s_row = l.s_row.as<uint32_t>(), *s_q = s_row + s1, *first = l.first.as<uint32_t>();
    uint32_t *pl = l.f3.as<uint32_t>(), *sc = pl + 3 * ((size_t)S + 1);
    uint32_t *chain_w = l.chain_w.as<uint32_t>(), *chain_q = l.chain_q.as<uint32_t>();
    uint64_t *x_rows = l.x_rows.as<uint64_t>(), *x_type = l.x_type.as<uint64_t>();
    CK(hipMemsetAsync(first, 0xFF, 4 * w1, s));
    if (S) {
        k_ls_spine<<<ls_blocks(S), kRvThreads, 0, s>>>(S, nk, sp_base, sp_op, key, off, elems, nw, vt.tk, vt.tv,
                                                       vt.tab_txn, vt.dir_bits, vt.dir, status, s_row, s_q, first,
                                                       level);
        CK(hipGetLastError());
    }
    k_ls_sflags<<<ls_blocks((size_t)S + 1), kRvThreads, 0, s>>>(S, s_row, first, vt.tab_txn, status, level, pl);
    CK(hipGetLastError());
    for (int q = 0; q < 4; ++q)
        CK(scan_exclusive_u32(pl + q * ((size_t)S + 1), (size_t)S + 1, tb.scratch.as<uint32_t>(), s));
    if (E) {
        k_ls_compare<<<ls_blocks(E), kRvThreads, 0, s>>>(E, n, off, elems, rk, sp_op, sp_len,
                                                         l.incompat.as<uint8_t>());
        CK(hipGetLastError());
    }
    if (S) {
        k_ls_chain<<<ls_blocks(S), kRvThreads, 0, s>>>(S, sc, s_row, s_q, vt.tab_txn, chain_w, chain_q);
        CK(hipGetLastError());
    }
    // fates, cid
    uint8_t *plane = l.plane.as<uint8_t>();
    CK(hipMemsetAsync(plane, 0, 2 * t1, s));
    k_ls_fate<<<ls_blocks((size_t)nt + 1), kRvThreads, 0, s>>>(nt, status, level, l.fate.as<uint8_t>(), f2, ct);
    CK(hipGetLastError());
    CK(scan_exclusive_u32(f2, (size_t)nt + 1, tb.scratch.as<uint32_t>(), s));
    uint32_t nc = 0, nch = 0;
    CK(hipMemcpyAsync(&nc, f2 + nt, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&nch, sc + S, 4, hipMemcpyDeviceToHost, s));
    if (nt) {
        k_ls_cid<<<ls_blocks(nt), kRvThreads, 0, s>>>(nt, level, f2, l.cid.as<uint32_t>(), l.txn_of.as<uint32_t>());
        CK(hipGetLastError());
    }
    // the edge rows: the reads' wr / rw slots, then the ww slots
    const uint32_t *cid = l.cid.as<uint32_t>();
    uint8_t *rflag = l.rflag.as<uint8_t>();
    k_ls_reads<<<ls_blocks(n + 1), kRvThreads, 0, s>>>(n, S, txn, off, rk, f1, l.incompat.as<uint8_t>(), sp_base, pl,
                                                       s_row, vt.tab_op, vt.tab_txn, chain_w, cid, rflag,
                                                       l.inck.as<uint8_t>(), plane, plane + t1, f0, x_rows, x_type,
                                                       ct);
    CK(hipGetLastError());
    if (S) {
        k_ls_ww<<<ls_blocks(S), kRvThreads, 0, s>>>(S, sc, chain_w, chain_q, cid, x_rows + 2 * nr, x_type + 2 * nr,
                                                    ct);
        CK(hipGetLastError());
    }
    // counts and the listed reads
    k_ls_txn_g1<<<ls_blocks(t1), kRvThreads, 0, s>>>(nt, plane, plane + t1, l.txn_g1.as<uint8_t>(), ct);
    CK(hipGetLastError());
    if (nk) {
        k_ls_inck<<<ls_blocks(nk), kRvThreads, 0, s>>>(nk, l.inck.as<uint8_t>(), ct);
        CK(hipGetLastError());
    }
    if (nw) {
        k_ls_unobs<<<ls_blocks(nw), kRvThreads, 0, s>>>(nw, vt.tab_txn, first, level, ct);
        CK(hipGetLastError());
    }
    CK(scan_exclusive_u32(f0, n + 1, tb.scratch.as<uint32_t>(), s));
    uint32_t nlist = 0, dup[kLsWords] = {};
    unsigned long long hct[kLcN] = {};
    CK(hipMemcpyAsync(&nlist, f0 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(hct, ct, 8 * kLcN, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(dup, tb.words_dev.p, 4 * kLsWords, hipMemcpyDeviceToHost, s));
    if (n) {
        k_ls_list<<<ls_blocks(n), kRvThreads, 0, s>>>(n, f0, rflag, HSC_RESOLVE_LIST_CAP, l.list_op.as<uint64_t>(),
                                                      l.list_flag.as<uint8_t>());
        CK(hipGetLastError());
    }
    CK(hipStreamSynchronize(s));
    if (dup[kLsDup]) {
        o.bad = 8;
        return hipErrorInvalidValue;
    }
    o.ncommitted = nc;
    o.chain_entries = nch;
    o.n_listed = std::min<uint32_t>(nlist, HSC_RESOLVE_LIST_CAP);
    o.g1a_reads = hct[kLcG1a];
    o.g1b_reads = hct[kLcG1b];
    o.dangling_reads = hct[kLcDangling];
    o.duplicate_reads = hct[kLcDupRd];
    o.incompatible_reads = hct[kLcIncompat];
    o.internal_reads = hct[kLcInternal];
    o.wr = hct[kLcWr];
    o.rw = hct[kLcRw];
    o.ww = hct[kLcWw];
    o.recovered = (uint32_t)hct[kLcRecovered];
    o.aborted = (uint32_t)hct[kLcAborted];
    o.dropped = (uint32_t)hct[kLcDropped];
    o.g1a_txns = (uint32_t)hct[kLcG1aTxns];
    o.g1b_txns = (uint32_t)hct[kLcG1bTxns];
    o.incompatible_keys = (uint32_t)hct[kLcIncKeys];
    o.unobserved_appends = hct[kLcUnobs];
    o.txn_of_cid.assign(nc, 0);
    o.listed_op.assign(o.n_listed, 0);
    o.listed_flag.assign(o.n_listed, 0);
    if (nt) {
        CK(hipMemcpyAsync(o.fate.data(), l.fate.p, nt, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.cid.data(), l.cid.p, 4 * (size_t)nt, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.txn_g1.data(), l.txn_g1.p, nt, hipMemcpyDeviceToHost, s));
    }
    if (nc) CK(hipMemcpyAsync(o.txn_of_cid.data(), l.txn_of.p, 4 * (size_t)nc, hipMemcpyDeviceToHost, s));
    if (o.n_listed) {
        CK(hipMemcpyAsync(o.listed_op.data(), l.list_op.p, 8 * (size_t)o.n_listed, hipMemcpyDeviceToHost, s));
        CK(hipMemcpyAsync(o.listed_flag.data(), l.list_flag.p, o.n_listed, hipMemcpyDeviceToHost, s));
    }
    if (arrays) {
        if (n) {
            o.rflag.resize(n);
            CK(hipMemcpyAsync(o.rflag.data(), rflag, n, hipMemcpyDeviceToHost, s));
        }
        if (nk) {
            o.spine_op.resize(nk);
            CK(hipMemcpyAsync(o.spine_op.data(), sp_op, 8 * (size_t)nk, hipMemcpyDeviceToHost, s));
        }
    }
    CK(hipStreamSynchronize(s));
    l.n_rows = n_rows;
    l.nc = nc;
    l.in_nops = n;
    l.in_ntxn = nt;
    l.valid = true;
    return hipSuccess;
}
#undef CK

// load this file's code object now (see warm_graph)
hipError_t warm_lists()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_ls_check);
}

}  // namespace hsc
