// hsc_narrow.hip -- the narrow window layout and its direct probe.
//
// The reference answers one read set at a time: for every logged write key it
// scans the read ranges of the written index with a min-length memcmp
// (db/glue.c:2937-2961).  When every (group, key) of the resident window fits
// one 64-bit code, this layout answers every range of a batch independently,
// with no bucketing of ranges at all:
//
//   key64[i] = (K_i - K_0) >> s     K = gid || word 0 || ... || word W-1 (the
//                                   composite sort key), K_0 = the first row;
//                                   s = the low bits every row agrees on
//                                   (trailing key words that never vary plus
//                                   tz low bits of the last one that does: a
//                                   9-byte int64 key, 0x08 || BE(v ^ 2^63),
//                                   has tz = 56).  Valid if the window spans
//                                   less than 2^62 << s -- any one int64 index.
//
// A probe bound X maps exactly to  rows >= X  <=>  key64 >= ceil((X - K_0) / 2^s)
// and  rows <= X  <=>  key64 <= floor((X - K_0) / 2^s), so the min-length
// memcmp range test of the reference becomes two counts over sorted u64s.
//
// Index: a 16-ary tree of key levels (level l+1 holds the last key of every
// 16-entry block of level l; one 128-byte line per block) and a parallel tree
// of commit-LSN maxima.  A group of 16 lanes answers one range: each lane
// reads one entry of the block, a ballot counts the entries below the bound,
// so every level costs one line and one ballot.  Upper levels live in LDS,
// the rest in L2 / the Infinity Cache (the window of BASELINE config 2 is
// 160 MB).  The range maximum then takes at most two partial blocks per level
// of the max tree.  Every group keeps kNP ranges (2 kNP searches) in flight.
#include "hsc_device.h"
#include "hsc_internal.h"
#include "hsc_reldiff.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

namespace hsc {

constexpr uint64_t kKeyPad = ~0ull;      // key padding: above every bound
// kSat (the saturated code: above every key), rel_diff, rel_diff_w and the
// fast instances' rel_short: hsc_reldiff.h

// Compressed codes (nv.comp): code(X) = compress(X over the rows' varying
// bits) - c0.  Rows map exactly; a bound X that leaves the rows' constant
// pattern maps by its first differing constant bit b (MSB first): with the
// varying bits above b as prefix, X is above every row of that prefix when
// its bit is 1 (#rows < X = #codes < (prefix + 1) << rest) and below them
// when 0 (#codes < prefix << rest) -- the compact codes' rule
// (hsc_compact_dev.h bound_word) on one word.  upper = false: the lower code
// (ceil: #codes < it = #rows < X), else the upper (floor: #codes <= it =
// #rows <= X); false = no row <= X (upper only).
__device__ __forceinline__ bool cnarrow_bound(const NarrowView &nv, uint64_t xg, const uint64_t *xw,
                                              size_t xs, bool upper, uint64_t &code)
{
    uint64_t acc = 0;
    int pos = 0, np = -1, xb = 0;
    for (int l = 0; l <= nv.W; ++l) {
        const uint64_t *cm = nv.cmeta + 8 * l;
        const uint64_t m = cm[0], pt = cm[1];
        uint64_t x = l ? xw[(size_t)(l - 1) * xs] : xg;
        if (np < 0) {
            const uint64_t d = (x ^ pt) & ~m;
            if (d) {
                const int b = 63 - __clzll(d);
                const uint64_t above = b == 63 ? 0 : ~0ull << (b + 1);
                np = pos + __popcll(m & above);
                xb = (int)((x >> b) & 1);
                x &= above;
            }
        } else {
            x = 0;
        }
        const int c = __popcll(m);
        if (c) {
            uint64_t mv[6];
#pragma unroll
            for (int q = 0; q < 6; ++q) mv[q] = cm[2 + q];
            acc = (c >= 64 ? 0 : acc << c) | bits_compress(x, m, mv);
            pos += c;
        }
    }
    uint64_t lo, hi;
    bool live = true;
    if (np < 0) {
        lo = hi = acc;
    } else {
        const int low = pos - np;
        const uint64_t pre = low >= 64 ? 0 : acc >> low;
        lo = (xb ? pre + 1 : pre) << low;
        live = lo != 0;
        hi = lo - 1;
    }
    if (upper) {
        if (!live || hi < nv.c0) return false;
        code = hi - nv.c0 < kSat ? hi - nv.c0 : kSat;
        return true;
    }
    code = lo <= nv.c0 ? 0 : (lo - nv.c0 < kSat ? lo - nv.c0 : kSat);
    return true;
}

// A probe bound as a code, either form: lower (ceil) / upper (floor); false
// (upper only) = no row at or below X.  Generic width (rel_diff).
__device__ __forceinline__ bool narrow_bound(const NarrowView &nv, uint64_t xg, const uint64_t *xw,
                                             size_t xs, bool upper, uint64_t &code)
{
    if (nv.comp) return cnarrow_bound(nv, xg, xw, xs, upper, code);
    uint64_t v;
    bool rem;
    if (!rel_diff(nv.W, nv.lw, nv.tz, xg, xw, xs, nv.base[0], nv.base + 1, 1, kSat, v, rem)) {
        code = 0;
        return !upper;  // below the window: lower 0, upper none
    }
    code = upper ? v : (v >= kSat ? kSat : v + (rem ? 1 : 0));
    return true;
}

bool narrow_span_fits(int W, int lw, int tz, const uint64_t *first, const uint64_t *last)
{
    uint64_t v;
    bool rem;
    if (!rel_diff(W, lw, tz, last[0], last + 1, 1, first[0], first + 1, 1, kSat, v, rem))
        return false;
    return !rem && v < kSat;
}

// ============================================================================
// window build
// ============================================================================
// rows 0 and n-1 as limbs (gid, words) -> out[0 .. W], out[W+1 .. 2W+1]
// (n_dev: the row count on the device, read there -- no host round trip)
__global__ void k_end_rows(WinView w, const uint32_t *n_dev, uint64_t *out)
{
    const int j = threadIdx.x;
    if (j > w.W) return;
    const uint32_t n = n_dev ? *n_dev : w.n;
    const size_t r[2] = {0, n ? (size_t)n - 1 : 0};
    for (int k = 0; k < 2; ++k)
        out[k * (w.W + 1) + j] =
            !n ? 0 : j ? w.words[(size_t)(j - 1) * w.stride + r[k]] : w.gid[r[k]];
}

hipError_t narrow_end_rows(const WinView &w, const uint32_t *n_dev, uint64_t *out, hipStream_t s)
{
    k_end_rows<<<1, 128, 0, s>>>(w, n_dev, out);
    return hipGetLastError();
}

namespace {
constexpr uint32_t kNoTile32 = 0xFFFFFFFFu;
constexpr int kTLog2 = 12;  // 4096-row tiles (= the code view's tiles)
constexpr int kRecentLog2 = 8;  // a tile's recent list: its R newest rows (k_recent)
constexpr uint32_t kRecent = 1u << kRecentLog2;  // R = 256
static_assert(kRecentLog2 < kTLog2 && kRecent == 4 * 64, "the join's wave 0 stages a list, a quad per lane");
}  // namespace

// Eytzinger (BFS) slot of sorted row r of a 4096-row tile: rows 0 .. 4094
// form a perfect binary tree at slots 1 .. 4095 (in-order index i = r + 1 sits
// at level 11 - ctz(i)), row 4095 at slot 0.  A root-to-leaf walk touches
// slots spread over a level instead of the power-of-two strides of a binary
// search over sorted rows, which all fall in one or two LDS banks.
static_assert(kTLog2 == 12, "eyt12 assumes 4096-row tiles");
__device__ __forceinline__ uint32_t eyt12(uint32_t r)
{
    const uint32_t i = r + 1;
    const int tz = __builtin_ctz(i);
    return i == 4096 ? 0 : (1u << (11 - tz)) + (i >> (tz + 1));
}

// level 0: key64 of every row (padding above n), lsn (padding 0)
__global__ void k_level0(WinView w, NarrowView nv, uint32_t len, uint64_t *key0, uint64_t *max0)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    uint64_t v = kKeyPad, m = 0;
    if (i < w.n) {
        bool rem;
        if (nv.comp)
            cnarrow_bound(nv, w.gid[i], w.words + i, w.stride, false, v);
        else
            rel_diff(w.W, nv.lw, nv.tz, w.gid[i], w.words + i, w.stride, nv.base[0], nv.base + 1, 1, kSat,
                     v, rem);
        m = w.lsn[i];
    }
    key0[i] = v;
    max0[i] = m;
}

// levels 0 and 1 in one pass: level 1's entry of every 16 rows from the 16
// lanes that hold them (last key, LSN maximum by shuffles) -- no second pass
// re-reading level 0's LSN column.  len0 is a multiple of the block size (whole
// tiles), level 1's entries past len0 / 16 are padding.
__device__ __forceinline__ uint64_t level0_key(const WinView &w, const NarrowView &nv, size_t i)
{
    uint64_t v = kKeyPad;
    bool rem;
    if (nv.comp)
        cnarrow_bound(nv, w.gid[i], w.words + i, w.stride, false, v);
    else
        rel_diff(w.W, nv.lw, nv.tz, w.gid[i], w.words + i, w.stride, nv.base[0], nv.base + 1, 1, kSat, v, rem);
    return v;
}

// The narrow tiles' rows from the same pass (narrow_build with key32): one
// 4096-row tile per workgroup, 4 rows per thread -- key32 = key64 - the tile's
// first key64, staged in LDS in the tile's Eytzinger order and stored
// coalesced; rank32 = LSN - base + 1 in lsn32 mode; *flag if a tile spans
// >= 2^32 (what k_key32 / k_rank_lsn32 write, without their passes over level 0)
struct Level01Tiles {
    uint32_t *key32, *rank32, *flag;
    uint64_t rank_base;
};

__global__ __launch_bounds__(256) void k_level01(WinView w, NarrowView nv, uint32_t len, uint64_t *key0,
                                                 uint64_t *max0, uint64_t *key1, uint64_t *max1, uint32_t len1)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t v = kKeyPad, m = 0;
    if (i < w.n) v = level0_key(w, nv, i), m = w.lsn[i];
    if (i < len) key0[i] = v, max0[i] = m;
    uint64_t mm = m;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const uint64_t y = __shfl_xor(mm, o, 16);
        mm = y > mm ? y : mm;
    }
    if ((i & 15) == 15 && i < len) key1[i >> 4] = v, max1[i >> 4] = mm;
    const size_t pad = len / 16 + i;
    if (pad < len1) key1[pad] = kKeyPad, max1[pad] = 0;
}

constexpr int kL01TThreads = 1024;
__global__ __launch_bounds__(kL01TThreads) void k_level01t(WinView w, NarrowView nv, uint32_t len,
                                                           uint64_t *key0, uint64_t *max0, uint64_t *key1,
                                                           uint64_t *max1, uint32_t len1, Level01Tiles T)
{
    constexpr int R = (1 << kTLog2) / kL01TThreads;
    __shared__ uint32_t st[1 << kTLog2];
    __shared__ uint64_t tfirst;
    const size_t base = (size_t)blockIdx.x << kTLog2;
    uint64_t v[R], m[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const size_t i = base + (size_t)k * kL01TThreads + threadIdx.x;
        v[k] = kKeyPad, m[k] = 0;
        if (i < w.n) v[k] = level0_key(w, nv, i), m[k] = w.lsn[i];
    }
    if (threadIdx.x == 0) tfirst = v[0];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const size_t i = base + (size_t)k * kL01TThreads + threadIdx.x;  // (< len: whole tiles)
        key0[i] = v[k], max0[i] = m[k];
        uint64_t mm = m[k];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const uint64_t y = __shfl_xor(mm, o, 16);
            mm = y > mm ? y : mm;
        }
        if ((i & 15) == 15) key1[i >> 4] = v[k], max1[i >> 4] = mm;
        if (T.rank32) T.rank32[i] = i < w.n ? (uint32_t)(m[k] - T.rank_base) + 1 : 0;
    }
    if (blockIdx.x == 0 && len / 16 + threadIdx.x < len1)
        key1[len / 16 + threadIdx.x] = kKeyPad, max1[len / 16 + threadIdx.x] = 0;
    __syncthreads();
    const uint64_t f = tfirst;
    bool wide = false;
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t r = k * kL01TThreads + threadIdx.x;
        uint32_t x = 0xFFFFFFFFu;
        if (base + r < w.n) {
            const uint64_t d = v[k] - f;
            wide |= d > 0xFFFFFFFFull;
            x = (uint32_t)d;
        }
        st[eyt12(r)] = x;
    }
    if (wide) atomicOr(T.flag, 1u);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const uint32_t r = k * kL01TThreads + threadIdx.x;
        T.key32[base + r] = st[r];
    }
}

// level l + 1 from level l: last key / max lsn of every 16-entry block
__global__ void k_level_up(const uint64_t *key_src, const uint64_t *max_src, uint32_t len_src,
                           uint64_t *key_dst, uint64_t *max_dst, uint32_t len_dst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len_dst) return;
    uint64_t k = kKeyPad, m = 0;
    if (i < len_src / 16) {
        k = key_src[16 * (size_t)i + 15];
        const ulonglong2 *src = (const ulonglong2 *)(max_src + 16 * (size_t)i);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const ulonglong2 v = src[j];
            m = v.x > m ? v.x : m;
            m = v.y > m ? v.y : m;
        }
    }
    key_dst[i] = k;
    max_dst[i] = m;
}

bool narrow_level01_tiles(const NarrowView &nv)
{
    return nv.levels >= 2 && nv.len[0] % (1u << kTLog2) == 0;
}

hipError_t narrow_build(const WinView &w, const NarrowView &nv, hipStream_t s, uint32_t *key32,
                        uint32_t *rank32, uint64_t rank_base, uint32_t *flag)
{
    const uint32_t len0 = nv.len[0];
    int l = 1;
    if (key32 && !narrow_level01_tiles(nv)) return hipErrorInvalidValue;
    if (nv.levels >= 2 && len0 % 256 == 0) {
        if (key32) {
            const hipError_t e = hipMemsetAsync(flag, 0, 4, s);
            if (e != hipSuccess) return e;
        }
        uint64_t *k1 = (uint64_t *)nv.keys + nv.off[1], *m1 = (uint64_t *)nv.maxs + nv.off[1];
        if (key32)
            k_level01t<<<len0 >> kTLog2, kL01TThreads, 0, s>>>(w, nv, len0, (uint64_t *)nv.keys, (uint64_t *)nv.maxs,
                                                               k1, m1, nv.len[1],
                                                               Level01Tiles{key32, rank32, flag, rank_base});
        else
            k_level01<<<len0 / 256, 256, 0, s>>>(w, nv, len0, (uint64_t *)nv.keys, (uint64_t *)nv.maxs, k1, m1,
                                                 nv.len[1]);
        l = 2;
    } else {
        k_level0<<<(len0 + 255) / 256, 256, 0, s>>>(w, nv, len0, (uint64_t *)nv.keys, (uint64_t *)nv.maxs);
    }
    for (; l < nv.levels; ++l)
        k_level_up<<<(nv.len[l] + 255) / 256, 256, 0, s>>>(
            nv.keys + nv.off[l - 1], nv.maxs + nv.off[l - 1], nv.len[l - 1],
            (uint64_t *)nv.keys + nv.off[l], (uint64_t *)nv.maxs + nv.off[l], nv.len[l]);
    return hipGetLastError();
}

// ============================================================================
// probe
// ============================================================================
constexpr int kProbeThreads = 256;
constexpr int kNP = 4;  // ranges per 16-lane group in flight

// A conflict mark.  kHost: the verdict bytes live in fine-grained host memory
// (the small-batch path) -- a system-scope store writes through to it, so the
// kernel's completion needs no L2 write-back.
template <bool kHost>
__device__ __forceinline__ void mark_verdict(uint8_t *v)
{
    if constexpr (kHost)
        __hip_atomic_store(v, (uint8_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else
        *v = 1;
}

// The ranges of p answered by 16-lane groups, kNP ranges each: wave w of the
// grid starts at range wave0 and strides by wstride.  Levels >= lds_from are
// read from top (LDS, lds_base = their offset), the rest from the window.
template <bool kHost = false>
__device__ __forceinline__ void narrow_probe_ranges(const NarrowView &nv, const ProbeView &p,
                                                    uint8_t *verdict, const uint64_t *top,
                                                    uint64_t lds_base, int lds_from,
                                                    uint32_t wave0, uint32_t wstride)
{
    const int lane = threadIdx.x & 63;
    const int sub = lane >> 4, l16 = lane & 15;
    const size_t ks = p.n;
    // every wave runs the same number of iterations (ballots need all lanes)
    for (uint32_t wbase = wave0; wbase < p.n; wbase += wstride) {
        const uint32_t base = wbase + sub * kNP;
        // lane k < kNP of the group maps range base + k to codes
        uint64_t mlo = kSat, mhi = 0, msnap = 0;
        uint32_t mtxn = 0;
        bool mlive = false;
        {
            const uint32_t q = base + l16;
            if (l16 < kNP && q < p.n) {
                const uint32_t g = p.gid[q];
                msnap = p.snap[q];
                mtxn = p.txn[q];
                // lower bound: ceil((lo - K0) >> s), 0 below the window;
                // upper bound: floor((hi - K0) >> s), none below the window
                narrow_bound(nv, g, p.lo + q, ks, false, mlo);
                mlive = narrow_bound(nv, g, p.hi + q, ks, true, mhi);
                if (!mlive) mhi = 0;
            }
        }
        uint64_t x[2 * kNP], snap[kNP];
        uint32_t txn[kNP];
        bool live[kNP];
#pragma unroll
        for (int k = 0; k < kNP; ++k) {
            const int src = (lane & 48) + k;
            x[2 * k] = __shfl(mlo, src, 64);
            x[2 * k + 1] = __shfl(mhi, src, 64);
            snap[k] = __shfl(msnap, src, 64);
            txn[k] = __shfl(mtxn, src, 64);
            live[k] = __shfl((int)mlive, src, 64) != 0;
        }
        // 2 kNP counts in lockstep: c[2k] = #keys < lo_k, c[2k+1] = #keys <= hi_k
        uint32_t c[2 * kNP];
#pragma unroll
        for (int j = 0; j < 2 * kNP; ++j) c[j] = 0;
        for (int l = nv.levels - 1; l >= 0; --l) {
            uint64_t e[2 * kNP];
            if (l >= lds_from) {
                const uint64_t *lv = top + (nv.off[l] - lds_base);
#pragma unroll
                for (int j = 0; j < 2 * kNP; ++j) e[j] = lv[16 * c[j] + l16];
            } else {
                const uint64_t *lv = nv.keys + nv.off[l];
#pragma unroll
                for (int j = 0; j < 2 * kNP; ++j) e[j] = lv[16 * (size_t)c[j] + l16];
            }
#pragma unroll
            for (int j = 0; j < 2 * kNP; ++j) {
                const bool below = (j & 1) ? e[j] <= x[j] : e[j] < x[j];
                const uint32_t m = (uint32_t)(__ballot(below) >> (16 * sub)) & 0xFFFFu;
                c[j] = 16 * c[j] + __popc(m);
            }
        }
        // any lsn > snapshot over rows [p, q): up the max tree, at most two
        // partial blocks per level
        uint32_t pp[kNP], qq[kNP];
        bool found[kNP];
#pragma unroll
        for (int k = 0; k < kNP; ++k) {
            pp[k] = c[2 * k];
            qq[k] = live[k] ? c[2 * k + 1] : 0;
            found[k] = false;
        }
        for (int l = 0; l < nv.levels; ++l) {
            bool more = false;
#pragma unroll
            for (int k = 0; k < kNP; ++k) more |= pp[k] < qq[k];
            if (!__any(more)) break;
            const uint64_t *lv = nv.maxs + nv.off[l];
            uint64_t vl[kNP], vr[kNP];
#pragma unroll
            for (int k = 0; k < kNP; ++k) {
                const bool act = pp[k] < qq[k];
                const uint32_t il = (pp[k] & ~15u) + l16;
                const uint32_t ir = ((qq[k] - 1) & ~15u) + l16;
                vl[k] = act && il >= pp[k] && il < qq[k] ? lv[il] : 0;
                vr[k] = act && ir >= pp[k] && ir < qq[k] ? lv[ir] : 0;
            }
#pragma unroll
            for (int k = 0; k < kNP; ++k) {
                const bool act = pp[k] < qq[k];
                const bool hit = vl[k] > snap[k] || vr[k] > snap[k];
                found[k] |= ((uint32_t)(__ballot(hit) >> (16 * sub)) & 0xFFFFu) != 0;
                const uint32_t np = (pp[k] + 15) >> 4, nq = qq[k] >> 4;
                const bool done = !act || found[k] || (pp[k] >> 4) == ((qq[k] - 1) >> 4) || np >= nq;
                pp[k] = done ? 0 : np;
                qq[k] = done ? 0 : nq;
            }
        }
        if (l16 == 0) {
#pragma unroll
            for (int k = 0; k < kNP; ++k)
                if (found[k]) mark_verdict<kHost>(verdict + txn[k]);
        }
    }
}

// table locks q = first, first + stride, ...: any write to a locked table
// after the snapshot
template <bool kHost = false>
__device__ __forceinline__ void narrow_probe_locks(const NarrowView &nv, const ProbeView &p,
                                                   uint8_t *verdict, uint32_t first, uint32_t stride)
{
    for (uint32_t q = first; q < p.n_lock; q += stride) {
        const uint32_t t = p.lock_table[q];
        if (t < nv.ntables && nv.table_max[t] > p.lock_snap[q]) mark_verdict<kHost>(verdict + p.lock_txn[q]);
    }
}

__global__ __launch_bounds__(kProbeThreads) void k_probe_narrow(NarrowView nv, ProbeView p,
                                                                uint8_t *verdict)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t top[];  // levels >= lds_from
    const uint64_t lds_base = nv.off[nv.lds_from];
    for (uint32_t i = threadIdx.x; i < nv.lds_entries; i += kProbeThreads)
        top[i] = nv.keys[lds_base + i];
    __syncthreads();
    const uint32_t groups = gridDim.x * (kProbeThreads / 16);
    const uint32_t wave0 = (blockIdx.x * (kProbeThreads / 16) + ((threadIdx.x >> 6) << 2)) * kNP;
    narrow_probe_ranges(nv, p, verdict, top, lds_base, nv.lds_from, wave0, groups * kNP);
    narrow_probe_locks(nv, p, verdict, blockIdx.x * kProbeThreads + threadIdx.x,
                       gridDim.x * kProbeThreads);
}

// Small batches of the drop-in entry (a lone bdb_osql_serial_check, a
// collector's batch of concurrent calls): one launch answers the ranges from
// the key and max trees (no LDS staging: a handful of searches would not pay
// for it), the delta run and the table locks.  The probe columns are read
// straight from the caller's pinned staging and the verdict bytes written into
// it (fine-grained host memory the GPU maps: no copies); the last block to
// finish stores `seq` into *done, which the host polls.  Completion needs no
// cache write-back: every verdict byte is a write-through system-scope store,
// each thread waits for its stores before the block counts itself done, and
// the done word is written (write-through, same path to the host) after the
// last block's count.
constexpr int kSmallThreads = 256;

// The small batches' range search, latency first: one range per 16-lane group
// (a lone call's ten ranges fill ten groups at once).  Lane 0 maps lo, lane 1
// hi.  The key tree is descended two levels per dependent step: the 256
// entries of level l - 1 under one entry of level l + 1 are contiguous (16 per
// lane, 2 KiB per group), so their count below the bound skips level l.  The
// range maximum needs no dependent chain at all: the partial blocks of every
// level follow from pa, pb by arithmetic, so kSmallRound levels' loads are
// issued together.
constexpr int kSmallRound = 4;
constexpr int kSmallLevels = kSmallMaxLevels;  // the host keeps deeper windows off this path
static_assert(kSmallLevels <= kMaxLevels, "level offsets");

__device__ __forceinline__ uint32_t group_sum16(uint32_t v)
{
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// #entries of the 16 at e (a lane's run of a level) below x (LE: <= x); none
// when the run starts at or past the level's end
template <bool LE>
__device__ __forceinline__ uint32_t run_below(const uint64_t *e, bool in, uint64_t x)
{
    if (!in) return 0;
    uint32_t n = 0;
#pragma unroll
    for (int i = 0; i < 16; i += 2) {
        const ulonglong2 v = *(const ulonglong2 *)(e + i);
        n += LE ? (v.x <= x) + (v.y <= x) : (v.x < x) + (v.y < x);
    }
    return n;
}

// KW = 1, 2: the bound's words loaded together into registers (they live in
// host memory: one PCIe round trip, not one per word) and mapped by
// rel_diff_w; KW = 0: any width through rel_diff
// a small batch's conflict mark: the verdict byte (system-scope store), or
// with vmask (a packed one-block batch) the read set's bit in LDS
__device__ __forceinline__ void small_mark(uint8_t *verdict, uint32_t *vmask, uint32_t txn)
{
    if (vmask)
        atomicOr(vmask, 1u << txn);
    else
        mark_verdict<true>(verdict + txn);
}

template <int KW>
__device__ __forceinline__ void narrow_small_ranges(const NarrowView &nv, const ProbeView &p,
                                                    uint8_t *verdict, uint32_t *vmask, uint32_t wave0,
                                                    uint32_t wstride)
{
    const int lane = threadIdx.x & 63, sub = lane >> 4, l16 = lane & 15, g0 = lane & 48;
    const size_t ks = p.n;
    for (uint32_t wbase = wave0; wbase < p.n; wbase += wstride) {
        const uint32_t q = wbase + sub;
        const bool act = q < p.n;
        uint64_t xv = 0, sn = 0;
        uint32_t tx = 0;
        int ok = 0;
        if (act && l16 < 2) {
            uint64_t v = 0;
            bool rem = false;
            const uint64_t *xp = l16 ? p.hi + q : p.lo + q;
            if (nv.comp) {  // compressed codes: the bound's code either way
                ok = narrow_bound(nv, p.gid[q], xp, ks, l16 != 0, v);
                xv = ok ? v : 0;
            } else {
                if constexpr (KW > 0) {
                    const uint32_t g = p.gid[q];
                    uint64_t xw[KW];
#pragma unroll
                    for (int j = 0; j < KW; ++j) xw[j] = xp[(size_t)j * ks];
                    ok = rel_diff_w<KW>(nv.lw, nv.tz, g, xw, nv.base[0], nv.base + 1, kSat, v, rem);
                } else {
                    ok = rel_diff(nv.W, nv.lw, nv.tz, p.gid[q], xp, ks, nv.base[0], nv.base + 1, 1, kSat,
                                  v, rem);
                }
                // lower bound: ceil((lo - K0) >> s), 0 below the window; upper:
                // floor((hi - K0) >> s), none below the window
                xv = !ok ? 0 : l16 ? v : (v >= kSat ? kSat : v + (rem ? 1 : 0));
            }
        } else if (act && l16 == 2) {
            sn = p.snap[q];
            tx = p.txn[q];
        }
        const uint64_t xlo = __shfl(xv, g0, 64), xhi = __shfl(xv, g0 + 1, 64);
        const bool live = act && __shfl(ok, g0 + 1, 64) != 0;
        const uint64_t snap = __shfl(sn, g0 + 2, 64);
        const uint32_t txn = __shfl(tx, g0 + 2, 64);
        // ca / cb: the block index at level l (the count below the bound at
        // l + 1).  Levels are compile-time indices (a window of < 2^32 rows
        // has at most kSmallLevels): every level's offset is a kernel-argument
        // load the prologue issues at once, not one per step.
        uint32_t ca = 0, cb = 0;
        const int top = nv.levels - 1;
#pragma unroll
        for (int l = kSmallLevels - 1; l >= 1; --l) {
            if (l > top || ((top - l) & 1)) continue;  // uniform
            const uint64_t *lv = nv.keys + nv.off[l - 1];
            const size_t len = nv.len[l - 1];
            const size_t ia = 256 * (size_t)ca + 16 * l16, ib = 256 * (size_t)cb + 16 * l16;
            const uint32_t na = run_below<false>(lv + ia, ia < len, xlo);
            const uint32_t nb = run_below<true>(lv + ib, ib < len, xhi);
            ca = 256 * ca + group_sum16(na);
            cb = 256 * cb + group_sum16(nb);
        }
        if ((top & 1) == 0) {  // level 0 left: a 16-ary step
            const uint64_t *lv = nv.keys;
            const bool ba = lv[16 * (size_t)ca + l16] < xlo, bb = lv[16 * (size_t)cb + l16] <= xhi;
            ca = 16 * ca + __popc((uint32_t)(__ballot(ba) >> (16 * sub)) & 0xFFFFu);
            cb = 16 * cb + __popc((uint32_t)(__ballot(bb) >> (16 * sub)) & 0xFFFFu);
        }
        // any lsn > snapshot over rows [P, Q): level L's partial blocks
        uint32_t P = ca, Q = live ? cb : 0;
        bool on = act && P < Q, found = false;
#pragma unroll
        for (int lev = 0; lev < kSmallLevels; lev += kSmallRound) {
            if (!__any(on)) break;
            uint64_t vl[kSmallRound], vr[kSmallRound];
#pragma unroll
            for (int r = 0; r < kSmallRound; ++r) {
                const int L = lev + r;
                const bool a = on && L < nv.levels;
                const uint64_t *lv = nv.maxs + nv.off[L];
                const uint32_t il = (P & ~15u) + l16, ir = ((Q - 1) & ~15u) + l16;
                vl[r] = a && il >= P && il < Q ? lv[il] : 0;
                vr[r] = a && ir >= P && ir < Q ? lv[ir] : 0;
                const uint32_t np = (P + 15) >> 4, nq = Q >> 4;
                on = a && (P >> 4) != ((Q - 1) >> 4) && np < nq;
                P = np, Q = nq;
            }
            bool hit = false;
#pragma unroll
            for (int r = 0; r < kSmallRound; ++r) hit |= vl[r] > snap || vr[r] > snap;
            found |= ((uint32_t)(__ballot(hit) >> (16 * sub)) & 0xFFFFu) != 0;
            on = on && !found;
        }
        if (act && found && l16 == 0) small_mark(verdict, vmask, txn);
    }
}

// ---- the appended rows: delta runs and the pending tail --------------------
// Keys as full composites (gid, W words) held in registers, W <= kPendMaxWords.

// row i of d below the key: (gid, words) < (g, k), or <= with !strict
template <int W>
__device__ __forceinline__ bool row_below(const DeltaView &d, uint32_t i, uint32_t g,
                                          const uint64_t (&k)[W], bool strict)
{
    const uint32_t rg = d.gid[i];
    uint64_t w[W];
#pragma unroll
    for (int j = 0; j < W; ++j) w[j] = d.words[(size_t)j * d.stride + i];
    if (rg != g) return rg < g;
#pragma unroll
    for (int j = 0; j < W; ++j)
        if (w[j] != k[j]) return w[j] < k[j];
    return !strict;
}

__device__ __forceinline__ bool group_any(bool x, int sub)
{
    return ((uint32_t)(__ballot(x) >> (16 * sub)) & 0xFFFFu) != 0;
}

// A 16-lane group (sub of the wave) asks: a row of d in [lo, hi] of group g
// committed after snap?  Both bounds come from 16-ary searches run in
// lockstep -- each round every lane reads one sample row, a ballot counts the
// samples below the bound and the interval shrinks 16-fold (4 rounds for a
// full 65536-row run, against 16 dependent steps of a binary search) -- then
// the LSNs between them 16 units at a time: rows at the ends, the 64-row
// maxima between.  Every lane of the wave runs the same rounds (ballots).
template <int W>
__device__ bool delta_range16(const DeltaView &d, bool act, uint32_t g, const uint64_t (&lo)[W],
                              const uint64_t (&hi)[W], uint64_t snap, int l16, int sub)
{
    uint32_t a0 = 0, al = act ? d.n : 0, b0 = 0, bl = al;  // count in [x0, x0 + xl]
    while (__any((al | bl) != 0)) {
        const uint32_t as = (al + 15) >> 4, bs = (bl + 15) >> 4;
        const uint32_t sa = (uint32_t)(l16 + 1) * as, sb = (uint32_t)(l16 + 1) * bs;
        const bool ab = al && sa <= al && row_below<W>(d, a0 + sa - 1, g, lo, true);
        const bool bb = bl && sb <= bl && row_below<W>(d, b0 + sb - 1, g, hi, false);
        const uint32_t ma = __popc((uint32_t)(__ballot(ab) >> (16 * sub)) & 0xFFFFu);
        const uint32_t mb = __popc((uint32_t)(__ballot(bb) >> (16 * sub)) & 0xFFFFu);
        if (al) {
            const uint32_t n0 = a0 + ma * as;
            al = min(as - 1, a0 + al - n0), a0 = n0;
        }
        if (bl) {
            const uint32_t n0 = b0 + mb * bs;
            bl = min(bs - 1, b0 + bl - n0), b0 = n0;
        }
    }
    // rows [pa, pb): h head rows, nb whole 64-row blocks, t tail rows
    const uint32_t pa = a0, pb = b0;
    uint32_t h = 0, nb = 0, t = 0, hend = pa, ts = pb;
    if (pa < pb) {
        hend = min(pb, (pa + 63) & ~63u);
        const uint32_t bend = pb & ~63u;
        nb = hend < bend ? (bend - hend) >> 6 : 0;
        ts = max(hend, bend);
        h = hend - pa, t = pb - ts;
    }
    const uint32_t U = h + nb + t;
    bool found = false;
    for (uint32_t k = 0; __any(k < U && !found); k += 16) {
        const uint32_t u = k + l16;
        bool hit = false;
        if (u < U && !found) {
            const uint64_t v = u < h        ? d.lsn[pa + u]
                               : u < h + nb ? d.bmax[(hend >> 6) + (u - h)]
                                            : d.lsn[ts + (u - h - nb)];
            hit = v > snap;
        }
        found |= group_any(hit, sub);
    }
    return found;
}

// the pending tail staged in LDS by every block of the second half
struct PendLds {
    uint32_t gid[kPendRows];
    uint64_t lsn[kPendRows];
    uint64_t words[kPendMaxWords][kPendRows];
    uint32_t ttid[kPendRows];
    uint64_t tlsn[kPendRows];
};

template <int W>
__device__ __forceinline__ bool pend_range16(const PendLds &s, uint32_t n, bool act, uint32_t g,
                                             const uint64_t (&lo)[W], const uint64_t (&hi)[W],
                                             uint64_t snap, int l16, int sub)
{
    bool hit = false;
    for (uint32_t r = l16; act && r < n; r += 16) {
        if (s.gid[r] != g || s.lsn[r] <= snap) continue;
        int cl = 0, ch = 0;  // sign of row - lo, row - hi (first differing word)
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const uint64_t w = s.words[j][r];
            if (!cl && w != lo[j]) cl = w < lo[j] ? -1 : 1;
            if (!ch && w != hi[j]) ch = w < hi[j] ? -1 : 1;
        }
        hit |= cl >= 0 && ch <= 0;
    }
    return group_any(hit, sub);
}

// The second half of k_small_narrow with W <= kPendMaxWords: a 16-lane group
// per range over the live run, a frozen one and the pending tail; a thread per
// table lock over the pending table maxima.
template <int W>
__device__ void small_appended16(const DeltaView &d, const DeltaView &d2, const PendView &pd,
                                 const ProbeView &p, uint8_t *verdict, uint32_t blk, uint32_t nblk)
{
    __shared__ PendLds s;
    if (pd.n || pd.nt) {
        const uint8_t *b = pd.base;
        for (uint32_t r = threadIdx.x; r < pd.n; r += kSmallThreads) {
            s.gid[r] = ((const uint32_t *)b)[r];
            s.lsn[r] = ((const uint64_t *)(b + kPendLsn))[r];
#pragma unroll
            for (int j = 0; j < W; ++j) s.words[j][r] = ((const uint64_t *)(b + kPendWords))[j * kPendRows + r];
        }
        for (uint32_t r = threadIdx.x; r < pd.nt; r += kSmallThreads) {
            s.ttid[r] = ((const uint32_t *)(b + kPendTtid))[r];
            s.tlsn[r] = ((const uint64_t *)(b + kPendTlsn))[r];
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, sub = lane >> 4, l16 = lane & 15;
    const uint32_t wave = blk * (kSmallThreads / 64) + (threadIdx.x >> 6);
    const uint32_t nwaves = nblk * (kSmallThreads / 64);
    for (uint32_t base = 4 * wave; base < p.n; base += 4 * nwaves) {
        const uint32_t q = base + sub;
        const bool act = q < p.n;
        uint32_t g = 0;
        uint64_t lo[W], hi[W], snap = 0;
#pragma unroll
        for (int j = 0; j < W; ++j) lo[j] = hi[j] = 0;
        if (act) {
            g = p.gid[q];
            snap = p.snap[q];
#pragma unroll
            for (int j = 0; j < W; ++j) lo[j] = p.lo[(size_t)j * p.n + q], hi[j] = p.hi[(size_t)j * p.n + q];
        }
        bool hit = false;
        if (d.n) hit |= delta_range16<W>(d, act, g, lo, hi, snap, l16, sub);
        if (d2.n) hit |= delta_range16<W>(d2, act && !hit, g, lo, hi, snap, l16, sub);
        if (pd.n) hit |= pend_range16<W>(s, pd.n, act && !hit, g, lo, hi, snap, l16, sub);
        if (act && hit && l16 == 0) mark_verdict<true>(verdict + p.txn[q]);
    }
    for (uint32_t q = blk * kSmallThreads + threadIdx.x; pd.nt && q < p.n_lock; q += nblk * kSmallThreads) {
        const uint32_t t = p.lock_table[q];
        const uint64_t ls = p.lock_snap[q];
        bool hit = false;
        for (uint32_t e = 0; e < pd.nt && !hit; ++e) hit = s.ttid[e] == t && s.tlsn[e] > ls;
        if (hit) mark_verdict<true>(verdict + p.lock_txn[q]);
    }
}

// WD = 0: keys wider than kPendMaxWords (no pending tail), a thread per range
// and binary searches; WD = 1..4: small_appended16<WD>.  KW: the window's
// search form (narrow_small_ranges<KW>), one per kernel (the code a launch
// runs stays small: its first instruction fetches are on the call's path).
template <int WD, int KW>
__global__ __launch_bounds__(kSmallThreads) void k_small_narrow(NarrowView nv, DeltaView d,
                                                                DeltaView d2, PendView pd,
                                                                ProbeView p, uint8_t *verdict,
                                                                uint32_t *blocks_done,
                                                                uint64_t *done, uint32_t seq, uint32_t pack)
{
    // with appended rows not in the window, the second half of the grid
    // searches them while the first half searches the window (both dependent
    // load chains run side by side instead of one after the other)
    const bool split = d.n || d2.n || pd.n || pd.nt;
    const uint32_t half = split ? gridDim.x / 2 : gridDim.x;
    __shared__ uint32_t vbits;
    const bool packed = pack && gridDim.x == 1;  // (split grids have two blocks at least)
    if (packed) {
        if (threadIdx.x == 0) vbits = 0;
        __syncthreads();
    }
    uint32_t *vmask = packed ? &vbits : nullptr;
    if (blockIdx.x < half) {
        const uint32_t groups = half * (kSmallThreads / 16);
        const uint32_t wave0 = blockIdx.x * (kSmallThreads / 16) + ((threadIdx.x >> 6) << 2);
        if (split) {  // (measured: the appended rows' half sets the pace; kNP ranges per group)
            narrow_probe_ranges<true>(nv, p, verdict, nullptr, 0, nv.levels, wave0 * kNP, groups * kNP);
        } else {
            narrow_small_ranges<KW>(nv, p, verdict, vmask, wave0, groups);
        }
        for (uint32_t q = blockIdx.x * kSmallThreads + threadIdx.x; q < p.n_lock; q += half * kSmallThreads) {
            const uint32_t t = p.lock_table[q];
            if (t < nv.ntables && nv.table_max[t] > p.lock_snap[q]) small_mark(verdict, vmask, p.lock_txn[q]);
        }
    } else if constexpr (WD > 0) {
        small_appended16<WD>(d, d2, pd, p, verdict, blockIdx.x - half, gridDim.x - half);
    } else {  // the live run and a frozen one (background fold)
        const uint32_t tid = (blockIdx.x - half) * kSmallThreads + threadIdx.x;
        const uint32_t nth = (gridDim.x - half) * kSmallThreads;
        for (uint32_t q = tid; q < p.n; q += nth)
            if ((d.n && delta_hit(d, p, q)) || (d2.n && delta_hit(d2, p, q)))
                mark_verdict<true>(verdict + p.txn[q]);
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this thread's verdict stores are done
    __syncthreads();
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {  // a lone call: no count to take; packed, the verdicts ride along
            const uint64_t w = (uint64_t)seq << 32 | (packed ? kSmallPacked | vbits : 0u);
            __hip_atomic_store(done, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        } else if (__hip_atomic_fetch_add(blocks_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                   gridDim.x - 1) {
            // the next launch of this slot counts from zero (stream order)
            __hip_atomic_store(blocks_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(done, (uint64_t)seq << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

hipError_t launch_small_narrow(const NarrowView &nv, const DeltaView &d, const DeltaView &d2,
                               const PendView &pd, const ProbeView &p,
                               uint8_t *verdict, uint32_t *blocks_done, uint64_t *done,
                               uint32_t seq, bool pack, hipStream_t s)
{
    // one pass of a range per 16-lane group, at most one block per CU (two
    // with appended rows pending: one per half of the grid)
    const bool split = d.n || d2.n || pd.n || pd.nt;
    const size_t per_block = (kSmallThreads / 16) * (split ? kNP : 1);
    const size_t work = std::max<size_t>({(p.n + per_block - 1) / per_block,
                                          (p.n_lock + kSmallThreads - 1) / kSmallThreads, 1});
    const unsigned blocks = (unsigned)(std::min<size_t>(work, 256) * (split ? 2 : 1));
    const int WD = split && nv.W <= kPendMaxWords ? nv.W : 0;
    if ((pd.n || pd.nt) && (WD == 0 || !pd.base || pd.n > kPendRows || pd.nt > kPendRows))
        return hipErrorInvalidValue;  // the host mirrors a tail only for W <= kPendMaxWords
    if ((d.n && d.W != nv.W) || (d2.n && d2.W != nv.W)) return hipErrorInvalidValue;
    const int KW = nv.W == 1 || nv.W == 2 ? nv.W : 0;
#define HSC_SMALL(WD_, KW_)                                                                              \
    k_small_narrow<WD_, KW_><<<blocks, kSmallThreads, 0, s>>>(nv, d, d2, pd, p, verdict, blocks_done, done, \
                                                              seq, pack)
#define HSC_SMALL_KW(WD_)                  \
    do {                                   \
        if (KW == 2)                       \
            HSC_SMALL(WD_, 2);             \
        else if (KW == 1)                  \
            HSC_SMALL(WD_, 1);             \
        else                               \
            HSC_SMALL(WD_, 0);             \
    } while (0)
    switch (WD) {
    case 1: HSC_SMALL_KW(1); break;
    case 2: HSC_SMALL_KW(2); break;
    case 3: HSC_SMALL_KW(3); break;
    case 4: HSC_SMALL_KW(4); break;
    default: HSC_SMALL_KW(0);
    }
#undef HSC_SMALL_KW
#undef HSC_SMALL
    return hipGetLastError();
}

hipError_t launch_probe_narrow(const NarrowView &nv, const ProbeView &p, uint8_t *verdict,
                               hipStream_t s)
{
    if (p.n == 0 && p.n_lock == 0) return hipSuccess;
    const size_t groups = (p.n + kNP - 1) / kNP;
    size_t blocks = (groups + kProbeThreads / 16 - 1) / (kProbeThreads / 16);
    blocks = std::max<size_t>(blocks, (p.n_lock + kProbeThreads - 1) / kProbeThreads);
    blocks = std::min<size_t>(std::max<size_t>(blocks, 1), 256 * 8);
    k_probe_narrow<<<(unsigned)blocks, kProbeThreads, (size_t)nv.lds_entries * 8 + 16, s>>>(
        nv, p, verdict);
    return hipGetLastError();
}

// Probe bounds -> codes (a one-word probe batch for the tile pipeline):
// lo64 = ceil((lo - K0) >> s), hi64 = floor((hi - K0) >> s); a range below
// the window gets lo64 = kSat > hi64 = 0 (empty).
__global__ void k_codes(NarrowView nv, ProbeView p, uint64_t *lo64, uint64_t *hi64)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= p.n) return;
    const uint32_t g = p.gid[q];
    uint64_t lo = 0, v = 0;
    narrow_bound(nv, g, p.lo + q, p.n, false, lo);
    const bool live = narrow_bound(nv, g, p.hi + q, p.n, true, v);
    lo64[q] = live ? lo : kSat;
    hi64[q] = live ? v : 0;
}

hipError_t narrow_codes(const NarrowView &nv, const ProbeView &p, uint64_t *lo64, uint64_t *hi64,
                        hipStream_t s)
{
    if (p.n == 0) return hipSuccess;
    k_codes<<<(p.n + 255) / 256, 256, 0, s>>>(nv, p, lo64, hi64);
    return hipGetLastError();
}


// ============================================================================
// narrow tiles: 4096-row tiles of (u32 key delta, u32 commit rank)
// ============================================================================
//
// For a dense batch the window is streamed once per batch, tile by tile,
// and the ranges are bucketed by tile (hist matrix + column scan, the plan
// of hsc_kernels.hip).  A row of a tile is 8 bytes:
//
//   key32[i]  = key64[i] - key64[first row of the tile]  (every tile spans
//               < 2^32 codes: checked at build, else the narrow window keeps
//               the code-tile pipeline)
//   rank32[i] = 1 + the index of the row's commit LSN among the window's
//               distinct commit LSNs C (sorted); a snapshot S maps to
//               r(S) = #{c in C : c <= S} and  lsn > S  <=>  rank > r(S).
//
// Join records are 16 bytes: {lo delta, hi delta, r(S), read set}.

__global__ void k_check_sorted(const uint64_t *v, size_t n, uint32_t *flag)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (i < n && v[i] < v[i - 1]) atomicOr(flag, 1u);
}

hipError_t check_sorted_u64(const uint64_t *v, size_t n, uint32_t *flag, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(flag, 0, 4, s);
    if (e != hipSuccess || n < 2) return e;
    k_check_sorted<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(v, n, flag);
    return hipGetLastError();
}

// rank32[i] = 1 + lower_bound(C, lsn[i]) (lsn[i] is in C); pads get 0.
// kRankK rows per thread searched in lockstep over the commit directory,
// whose upper levels are staged in LDS (defined with the locate kernel).
constexpr int kRankThreads = 1024, kRankK = 8;
__host__ __device__ inline uint32_t dir16_lds_entries(const Dir16 &d);
__global__ __launch_bounds__(kRankThreads) void k_rank32(const uint64_t *lsn, uint32_t n,
                                                         uint32_t len, Dir16 d, uint32_t *rank);


// key32 = key64 - first key64 of the tile, stored in the tile's Eytzinger
// order (the join copies a tile's keys into LDS as they lie); flag := 1 if a
// tile spans >= 2^32
__global__ void k_key32(const uint64_t *key64, uint32_t n, uint32_t len, uint32_t *key32,
                        uint32_t *flag)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const uint32_t dst = (i & ~((1u << kTLog2) - 1)) + eyt12(i & ((1u << kTLog2) - 1));
    if (i >= n) {
        key32[dst] = 0xFFFFFFFFu;
        return;
    }
    const uint64_t d = key64[i] - key64[(size_t)(i >> kTLog2) << kTLog2];
    if (d > 0xFFFFFFFFull) atomicOr(flag, 1u);
    key32[dst] = (uint32_t)d;
}

// lsn32 mode: rank32 = lsn - base + 1 (pads 0)
__global__ void k_rank_lsn32(const uint64_t *lsn, uint32_t n, uint32_t len, uint64_t base,
                             uint32_t *rank)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) rank[i] = i < n ? (uint32_t)(lsn[i] - base) + 1 : 0;
}

hipError_t narrow_tiles_build(const uint64_t *key64, const uint64_t *lsn, uint32_t n, uint32_t len,
                              const Dir16 &cdir, int rank_lsn32, uint64_t rank_base,
                              uint32_t *key32, uint32_t *rank32, uint32_t *flag, hipStream_t s)
{
    if (!flag) {  // (key32 and the flag written by the level pass: the ranks only)
        if (len == 0 || rank_lsn32) return hipSuccess;
    } else {
        hipError_t e = hipMemsetAsync(flag, 0, 4, s);
        if (e != hipSuccess || len == 0) return e;
        k_key32<<<(len + 255) / 256, 256, 0, s>>>(key64, n, len, key32, flag);
    }
    if (rank_lsn32) {
        k_rank_lsn32<<<(len + 255) / 256, 256, 0, s>>>(lsn, n, len, rank_base, rank32);
    } else {
        const uint32_t per = kRankThreads * kRankK;
        k_rank32<<<(len + per - 1) / per, kRankThreads, 8 * dir16_lds_entries(cdir), s>>>(
            lsn, n, len, cdir, rank32);
    }
    return hipGetLastError();
}

// ---- recent lists ----
// The kRecent (R) newest rows of every tile, for the join (join_s_item):
//   members  the min(R, tn) rows of the tile's tn with the largest rank32; ties
//            at the cut go to the smaller key (the earlier row);
//   rkey32   their key32 in key order, laid out as a 256-entry Eytzinger tree
//            (sorted position i at eyt8(i)); rrank32 their ranks in key order;
//            a short list is padded with key ~0 and rank 0 (row ranks start at
//            1), so a pad is above every bound and older than every snapshot;
//   rtheta   the largest rank32 of a row left out, 0 if none is.
// Every row of the tile with rank32 > rtheta is a member (a row left out has
// rank <= rtheta), which is all the join needs to know.
// One workgroup per tile, after key32 / rank32 are final (either rank mode):
// thread t holds rows 4t .. 4t + 3 (ranks lie in row order), the R-th largest
// rank is selected bit by bit from the top (a block count per bit), the rows
// equal to it and then the members are numbered by block scans in row order.
__device__ __forceinline__ uint32_t eyt8(uint32_t r)
{
    const uint32_t i = r + 1;
    const int tz = __builtin_ctz(i);
    return i == kRecent ? 0 : (1u << (kRecentLog2 - 1 - tz)) + (i >> (tz + 1));
}

constexpr int kRecentThreads = (1 << kTLog2) / 4;
// exclusive scan of x over the block's threads; ws: a wave-total array of its own
__device__ __forceinline__ uint32_t recent_scan(uint32_t x, uint32_t *ws)
{
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t s = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(s, o, 64);
        if (lane >= (uint32_t)o) s += y;
    }
    if (lane == 63) ws[wave] = s;
    __syncthreads();
    uint32_t run = s - x;
    for (uint32_t w = 0; w < wave; ++w) run += ws[w];
    return run;
}

// The tile's slot table from the same staged rows: smax[key32 >> shift] takes
// the row's rank by an LDS max, and slot i of the tile is stored as
// smax[i] >> qshift (NarrowTiles::slots; join records the locate may drop).
// The tile's span comes from the first codes, as the locate derives it.
__device__ __forceinline__ uint64_t slot_span(const uint64_t *first, uint32_t tile, uint32_t ntiles)
{
    const uint64_t sp = tile + 1 < ntiles ? first[tile + 1] - first[tile] : 1ull << 32;
    return sp > (1ull << 32) ? 1ull << 32 : sp;
}

__global__ __launch_bounds__(kRecentThreads) void k_recent(const uint32_t *key32, const uint32_t *rank32,
                                                           uint32_t n, uint32_t *rkey32, uint32_t *rrank32,
                                                           uint32_t *rtheta, const uint64_t *first,
                                                           int qshift, uint16_t *slots)
{
    constexpr uint32_t T = 1u << kTLog2;
    static_assert(kSlots <= kRecentThreads, "a slot per thread");
    __shared__ __attribute__((aligned(16))) uint32_t sk[T];  // the tile's keys as stored (eyt12 order)
    __shared__ uint32_t cnt[32], ws[2][kRecentThreads / 64], lk[kRecent], lr[kRecent], theta;
    __shared__ uint32_t smax[kSlots];
    const uint32_t tile = blockIdx.x, t = threadIdx.x, lane = t & 63;
    const size_t ts = (size_t)tile << kTLog2;
    const uint32_t tn = min(T, n - (tile << kTLog2));
    const u32x4 rq = *(const u32x4 *)(rank32 + ts + 4 * t);
    ((u32x4 *)sk)[t] = *(const u32x4 *)(key32 + ts + 4 * t);
    const int shift = narrow_slot_shift(slot_span(first, tile, gridDim.x));
    const uint32_t rv[4] = {rq.x, rq.y, rq.z, rq.w};
    if (t < 32) cnt[t] = 0;
    if (t < kRecent) lk[t] = 0xFFFFFFFFu, lr[t] = 0;
    if (t < kSlots) smax[t] = 0;
    if (t == 0) theta = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * t + k < tn) atomicMax(&smax[min(sk[eyt12(4 * t + k)] >> shift, kSlots - 1)], rv[k]);
    // v = the R-th largest rank, take = how many of the rows equal to v are
    // members (tn <= R: every row is one -- pads have rank 0, rows >= 1)
    uint32_t v = 0, take = kRecent;
    if (tn > kRecent) {
        for (int b = 31; b >= 0; --b) {
            // rows that agree with v above bit b and have bit b set
            const uint32_t want = v >> b | 1;
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) c += (rv[k] >> b) == want;
#pragma unroll
            for (int o = 32; o; o >>= 1) c += __shfl_xor(c, o, 64);
            if (lane == 0 && c) atomicAdd(&cnt[b], c);
            __syncthreads();
            const uint32_t c1 = cnt[b];
            if (c1 >= take)
                v |= 1u << b;
            else
                take -= c1;
        }
    }
    bool eq[4];
    uint32_t ne = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) eq[k] = 4 * t + k < tn && rv[k] == v, ne += eq[k];
    uint32_t ei = recent_scan(ne, ws[0]);
    bool mem[4];
    uint32_t nm = 0, out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        mem[k] = 4 * t + k < tn && (rv[k] > v || (eq[k] && ei < take));
        ei += eq[k];
        nm += mem[k];
        if (4 * t + k < tn && !mem[k]) out = max(out, rv[k]);
    }
    uint32_t pos = recent_scan(nm, ws[1]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (mem[k]) {
            lk[eyt8(pos)] = sk[eyt12(4 * t + k)];
            lr[pos] = rv[k];
            ++pos;
        }
#pragma unroll
    for (int o = 32; o; o >>= 1) out = max(out, (uint32_t)__shfl_xor((int)out, o, 64));
    if (lane == 0 && out) atomicMax(&theta, out);
    __syncthreads();
    if (t < kRecent) {
        rkey32[(size_t)tile * kRecent + t] = lk[t];
        rrank32[(size_t)tile * kRecent + t] = lr[t];
    }
    if (t == 0) rtheta[tile] = theta;
    if (t < kSlots) slots[(size_t)tile * kSlots + t] = (uint16_t)(smax[t] >> qshift);
}

// lists, rtheta, then the slot tables (kSlots u16 per tile)
size_t narrow_recent_words(uint32_t ntiles) { return (size_t)ntiles * (2 * kRecent + 1 + kSlots / 2); }

hipError_t narrow_recent_build(const uint32_t *key32, const uint32_t *rank32, uint32_t n, uint32_t ntiles,
                               const uint64_t *first, int qshift, uint32_t *recent, hipStream_t s)
{
    if (ntiles == 0) return hipSuccess;
    uint32_t *rkey = recent, *rrank = rkey + (size_t)ntiles * kRecent, *rtheta = rrank + (size_t)ntiles * kRecent;
    k_recent<<<ntiles, kRecentThreads, 0, s>>>(key32, rank32, n, rkey, rrank, rtheta, first, qshift,
                                               (uint16_t *)(rtheta + ntiles));
    return hipGetLastError();
}

void narrow_recent_view(NarrowTiles &nt, const uint32_t *recent, uint32_t ntiles, int qshift)
{
    nt.rkey32 = recent;
    nt.rrank32 = recent + (size_t)ntiles * kRecent;
    nt.rtheta = nt.rrank32 + (size_t)ntiles * kRecent;
    nt.slots = (const uint16_t *)(nt.rtheta + ntiles);
    nt.qshift = qshift;
}

// ---- 16-ary directories over sorted u64 arrays ----
__global__ void k_dir_level0(const uint64_t *src, uint32_t n, uint32_t len, uint64_t *dst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) dst[i] = i < n ? src[i] : ~0ull;
}

__global__ void k_dir_up(const uint64_t *src, uint32_t len_src, uint64_t *dst, uint32_t len_dst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len_dst) dst[i] = i < len_src / 16 ? src[16 * (size_t)i + 15] : ~0ull;
}

hipError_t dir16_build(const uint64_t *src, uint32_t n, DBuf &buf, Dir16 &d, uint32_t max_lds,
                       hipStream_t s)
{
    d = Dir16{};
    d.n = n;
    uint32_t len = (n + 16) & ~15u;  // at least one pad: every level ends in ~0
    uint64_t off = 0;
    int L = 0;
    for (;;) {
        if (L == kDirLevels) return hipErrorInvalidValue;
        d.off[L] = (uint32_t)off;
        d.len[L] = len;
        off += len;
        ++L;
        if (len <= 16) break;
        len = ((len / 16) + 15) & ~15u;
    }
    d.levels = L;
    d.lds_from = L - 1;
    d.lds_n = d.len[L - 1];
    while (d.lds_from > 0 && d.lds_n + d.len[d.lds_from - 1] <= max_lds) d.lds_n += d.len[--d.lds_from];
    hipError_t e = buf.ensure(8 * off);
    if (e != hipSuccess) return e;
    uint64_t *v = buf.as<uint64_t>();
    d.v = v;
    k_dir_level0<<<(d.len[0] + 255) / 256, 256, 0, s>>>(src, n, d.len[0], v);
    for (int l = 1; l < L; ++l)
        k_dir_up<<<(d.len[l] + 255) / 256, 256, 0, s>>>(v + d.off[l - 1], d.len[l - 1],
                                                          v + d.off[l], d.len[l]);
    return hipGetLastError();
}

// Upper levels [lds_from, levels) of a directory into LDS, every 16-entry
// block at a 17-entry stride: entry e of block c sits at 17 c + e, so the
// same entry of different blocks falls in different banks (at a 16-entry
// stride entries 3 / 7 / 11 of every block share two of the 64 banks).
constexpr uint32_t kDirLdsStride = 17;
__host__ __device__ inline uint32_t dir16_lds_entries(const Dir16 &d)
{
    return d.lds_n / 16 * kDirLdsStride;
}
__device__ __forceinline__ void dir16_stage(const Dir16 &d, uint64_t *lds)
{
    const uint64_t *src = d.v + d.off[d.lds_from];
    for (uint32_t i = threadIdx.x; i < d.lds_n; i += blockDim.x)
        lds[(i >> 4) * kDirLdsStride + (i & 15)] = src[i];
}

// One level of a 16-ary directory for K keys in lockstep: c[k] (block index
// at this level) becomes 16 c[k] + #{entries of the block below xx[k]}.  Two
// rounds of three independent reads (entries 3, 7, 11 pick the quarter, then
// its first three entries) instead of a 4-step dependent chain.  A block's
// last entry is never below a key (levels end in ~0 padding and a block's last
// entry bounds the key one level up), so the count fits 0..15.
template <int K, uint32_t STRIDE = 16>
__device__ __forceinline__ void dir16_level(const uint64_t *lv, const uint64_t (&xx)[K],
                                            uint32_t (&c)[K])
{
    uint32_t qd[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t *b = lv + STRIDE * c[k];
        qd[k] = (uint32_t)(b[3] < xx[k]) + (uint32_t)(b[7] < xx[k]) + (uint32_t)(b[11] < xx[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t *b = lv + STRIDE * c[k] + 4 * qd[k];
        c[k] = 16 * c[k] + 4 * qd[k] + (uint32_t)(b[0] < xx[k]) + (uint32_t)(b[1] < xx[k]) +
               (uint32_t)(b[2] < xx[k]);
    }
}

// Strict bound for "entries <= x" (entries are < ~0: ~0 is padding).
__device__ __forceinline__ uint64_t dir_le(uint64_t x) { return x >= ~0ull - 1 ? ~0ull : x + 1; }

// out[k] = #{entries < xx[k]} (0 where act[k] is false).  Levels held in LDS
// and levels in global memory run as separate loops so that every read has
// a known address space (no flat loads).
template <int K>
__device__ __forceinline__ void dir16_count(const Dir16 &d, const uint64_t *lds,
                                            const uint64_t (&xx)[K], const bool (&act)[K],
                                            uint32_t (&out)[K])
{
    uint32_t c[K];
#pragma unroll
    for (int k = 0; k < K; ++k) c[k] = 0;
    const uint32_t lds_base = d.off[d.lds_from];
    for (int l = d.levels - 1; l >= d.lds_from; --l)
        dir16_level<K, kDirLdsStride>(lds + (d.off[l] - lds_base) / 16 * kDirLdsStride, xx, c);
    for (int l = d.lds_from - 1; l >= 0; --l) dir16_level<K>(d.v + d.off[l], xx, c);
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = act[k] ? min(c[k], d.n) : 0;
}

__global__ __launch_bounds__(kRankThreads) void k_rank32(const uint64_t *lsn, uint32_t n,
                                                         uint32_t len, Dir16 d, uint32_t *rank)
{
    extern __shared__ __attribute__((aligned(16))) uint64_t rlds[];
    const uint32_t i0 = blockIdx.x * (kRankThreads * kRankK) + threadIdx.x;
    uint64_t x[kRankK];
    bool act[kRankK];
#pragma unroll
    for (int k = 0; k < kRankK; ++k) {
        const uint32_t i = i0 + k * kRankThreads;
        act[k] = i < n;
        x[k] = act[k] ? lsn[i] : 0;
    }
    dir16_stage(d, rlds);
    __syncthreads();
    uint32_t c[kRankK];
    dir16_count<kRankK>(d, rlds, x, act, c);
#pragma unroll
    for (int k = 0; k < kRankK; ++k) {
        const uint32_t i = i0 + k * kRankThreads;
        if (i < len) rank[i] = act[k] ? c[k] + 1 : 0;
    }
}

// ---- locate: codes, snapshot ranks, end tiles, per-chunk tile histogram ----
// One workgroup per chunk of kLocTP * kLocTThreads probes; thread t owns
// probes c0 + t + kLocTThreads j, j < kLocTP (consecutive lanes =
// consecutive probes, so a read set's ranges sit in neighbouring lanes).
// Every probe load is issued up front; the tile and snapshot-rank searches
// run for all kLocTP probes in lockstep over 16-ary directories whose upper
// levels are staged in LDS (kTileLds: the whole tile directory, so the tile
// search and the tiles' first codes never leave LDS).  Output per probe: its
// first join record {tile << 12 | rank, lo, hi, r(S)} and, for a range that
// spans two tiles, its second one.
constexpr int kLocTP = 4;
constexpr int kLocTThreads = 1024;  // <= 4096 probes per chunk (in-chunk ranks fit 12 bits)
static_assert(kLocTP * kLocTThreads <= 4096, "in-chunk ranks are 12 bits");
constexpr int kDirLds = 4400;  // directory entries staged in LDS per directory
// k_locate_t stages a directory from registers: 16-byte pieces (two entries) per thread
constexpr int kDirSlots = ((kDirLds + 1) / 2 + kLocTThreads - 1) / kLocTThreads;  // 3
static_assert((kDirLds + 1) / 2 <= kDirSlots * kLocTThreads, "directory slots of k_locate_t");

// dir16_stage in two halves for a workgroup of THREADS: every load issued
// into registers (a slot past the directory reads piece 0 again), then,
// after whatever the caller overlaps with the loads, the LDS stores.  lds_n
// is a multiple of 16, so a piece never straddles a block; the 17-entry
// stride leaves the LDS side 8-byte stores.
template <int THREADS, int SLOTS>
__device__ __forceinline__ void dir16_stage_issue(const Dir16 &d, u64x2 (&v)[SLOTS])
{
    const u64x2 *src = (const u64x2 *)(d.v + d.off[d.lds_from]);
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const uint32_t i = threadIdx.x + THREADS * j;
        v[j] = src[i < d.lds_n / 2 ? i : 0];
    }
}
template <int THREADS, int SLOTS>
__device__ __forceinline__ void dir16_stage_store(const Dir16 &d, const u64x2 (&v)[SLOTS],
                                                  uint64_t *lds)
{
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
        const uint32_t i = threadIdx.x + THREADS * j;
        if (i < d.lds_n / 2) {
            uint64_t *o = lds + (i >> 3) * kDirLdsStride + 2 * (i & 7);
            o[0] = v[j].x;
            o[1] = v[j].y;
        }
    }
}

template <int W>
__device__ __forceinline__ void locate_codes(const NarrowView &nv, const ProbeView &p, uint32_t q,
                                             uint64_t g, const uint64_t (&xl)[2 > W ? 2 : W],
                                             const uint64_t (&xh)[2 > W ? 2 : W], uint64_t &lo,
                                             uint64_t &hi)
{
    uint64_t v = 0;
    bool rem;
    uint64_t a = 0;
    bool live;
    if (nv.comp) {  // compressed codes (the loaded words live at p.lo / p.hi + q too)
        narrow_bound(nv, g, p.lo + q, p.n, false, a);
        live = narrow_bound(nv, g, p.hi + q, p.n, true, v);
    } else if constexpr (W > 0) {
        const uint64_t(&wl)[W] = *(const uint64_t(*)[W])xl;
        const uint64_t(&wh)[W] = *(const uint64_t(*)[W])xh;
        a = rel_diff_w<W>(nv.lw, nv.tz, g, wl, nv.base[0], nv.base + 1, kSat, v, rem)
                ? (v >= kSat ? kSat : v + (rem ? 1 : 0))
                : 0;
        live = rel_diff_w<W>(nv.lw, nv.tz, g, wh, nv.base[0], nv.base + 1, kSat, v, rem);
    } else {
        a = rel_diff(nv.W, nv.lw, nv.tz, g, p.lo + q, p.n, nv.base[0], nv.base + 1, 1, kSat, v,
                     rem)
                ? (v >= kSat ? kSat : v + (rem ? 1 : 0))
                : 0;
        live = rel_diff(nv.W, nv.lw, nv.tz, g, p.hi + q, p.n, nv.base[0], nv.base + 1, 1, kSat, v,
                        rem);
    }
    lo = live ? a : kSat;  // a range below the window is empty
    hi = live ? v : 0;
}

// locate_codes of the fast instances (no compressed codes, lw == W): the
// wave takes the short mapping (hsc_reldiff.h rel_short) when both bounds of
// every lane meet its precondition -- a lane without a probe counts as
// meeting it, its codes are never used -- and rel_diff_w otherwise, whole, so
// the choice is a uniform branch.  bs = the base's limbs, read once.
template <int W>
__device__ __forceinline__ void locate_codes_fast(int tz, const uint64_t (&bs)[W + 1], bool valid,
                                                  uint64_t g, const uint64_t (&xl)[2],
                                                  const uint64_t (&xh)[2], uint64_t &lo,
                                                  uint64_t &hi)
{
    const uint64_t(&wl)[W] = *(const uint64_t(*)[W])xl;
    const uint64_t(&wh)[W] = *(const uint64_t(*)[W])xh;
    const bool fits = !valid || (rel_short_ok<W>(tz, g, wl, bs[0], bs + 1) &&
                                 rel_short_ok<W>(tz, g, wh, bs[0], bs + 1));
    uint64_t v = 0, a = 0;
    bool rem, live;
    if (__ballot(fits) == ~0ull) {
        a = rel_short<W>(tz, wl, bs + 1, kSat, v, rem) ? (v >= kSat ? kSat : v + (rem ? 1 : 0)) : 0;
        live = rel_short<W>(tz, wh, bs + 1, kSat, v, rem);
    } else {
        a = rel_diff_w<W>(W, tz, g, wl, bs[0], bs + 1, kSat, v, rem)
                ? (v >= kSat ? kSat : v + (rem ? 1 : 0))
                : 0;
        live = rel_diff_w<W>(W, tz, g, wh, bs[0], bs + 1, kSat, v, rem);
    }
    lo = live ? a : kSat;  // a range below the window is empty
    hi = live ? v : 0;
}

// ---- bucket table over the tiles' first codes ----
// first[0] = 0 (codes are relative to the window's first row), so bucket k
// covers codes [k << shift, (k + 1) << shift) with shift the least that puts
// the last tile's first code below m << shift.  trad[k] = #first < k << shift
// for k <= m; trad[m + 1] = shift.
constexpr uint32_t kTradMaxTiles = 4096;   // first codes staged in LDS (32 KiB)
constexpr uint32_t kTradMax = 4096;        // buckets (u16 in LDS: 8 KiB)
// k_locate_t stages both from registers: 16-byte pieces per thread
constexpr int kTradFirstSlots = kTradMaxTiles / 2 / kLocTThreads;  // first codes: 2
constexpr int kTradSlots = ((kTradMax + 1 + 7) / 8 + kLocTThreads - 1) / kLocTThreads;  // packed table: 1
static_assert(kTradMaxTiles / 2 <= kTradFirstSlots * kLocTThreads, "first-code slots of k_locate_t");
static_assert((kTradMax + 1 + 7) / 8 <= kTradSlots * kLocTThreads, "bucket-table slots of k_locate_t");
uint32_t narrow_trad_buckets(uint32_t ntiles, bool force_dir)
{
    if (force_dir || ntiles == 0 || ntiles > kTradMaxTiles) return 0;  // force_dir: tests
    uint32_t m = 16;
    while (m < 2 * ntiles && m < kTradMax) m *= 2;
    return m;
}

// Log mode (trad[m + 1] = kTradLog | s, m = 64 << s): bucket of x = its
// exponent and s mantissa bits, like a float -- monotone, with the resolution
// where the codes are dense near zero (hot keys of a Zipf window crowd a few
// linear buckets); the build picks the mode whose fullest bucket holds fewer
// tiles (narrow_trad_pick).
__global__ void k_trad(const uint64_t *first, uint32_t ntiles, uint32_t m, int logmode,
                       uint32_t *trad, uint16_t *trad16)
{
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    // the packed copy's padding (entries m + 1 .. of its last 16-byte piece)
    if (k > m && k < narrow_trad16_bytes(m) / 2) trad16[k] = 0;
    if (k > m + 1) return;
    // entry k <= m of both tables (a count of tiles: <= kTradMaxTiles, so it fits u16)
    auto put = [&](uint32_t v) {
        trad[k] = v;
        trad16[k] = (uint16_t)v;
    };
    const int lg = 31 - __clz(m);
    if (logmode) {
        const int sv = lg - 6;
        if (k == m + 1) {
            trad[k] = kTradLog | (uint32_t)sv;
            return;
        }
        uint32_t lo = 0, hi = ntiles;  // #tiles whose first code's bucket < k
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (trad_log_bucket(first[mid], sv) < k)
                lo = mid + 1;
            else
                hi = mid;
        }
        put(lo);
        return;
    }
    const uint64_t span = first[ntiles - 1];
    const int bits = span ? 64 - __clzll(span) : 0;
    const int shift = bits > lg ? bits - lg : 0;
    if (k == m + 1) {
        trad[k] = (uint32_t)shift;
        return;
    }
    if (k == m) {  // every first code is below m << shift (which overflows when span >= 2^63)
        put(ntiles);
        return;
    }
    const uint64_t x = (uint64_t)k << shift;
    uint32_t lo = 0, hi = ntiles;  // #first < x
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    put(lo);
}

static_assert(kTradMaxTiles <= 0xFFFF, "the packed table holds tile counts as u16");

hipError_t narrow_trad_build(const uint64_t *first, uint32_t ntiles, uint32_t m, uint32_t *trad,
                             uint16_t *trad16, hipStream_t s, int logmode)
{
    if (logmode && m < 64) return hipErrorInvalidValue;
    if (ntiles > kTradMaxTiles) return hipErrorInvalidValue;
    // threads 0 .. m + 1 for the u32 table, up to m + 7 for the packed copy's padding
    k_trad<<<(m + 8 + 255) / 256, 256, 0, s>>>(first, ntiles, m, logmode, trad, trad16);
    return hipGetLastError();
}

// LDS carve of k_locate_t (same on host and device).  Tile bucket mode:
// first codes [ntiles] + cdir levels + histogram [ntiles] + bucket table u16
// [m + 1] + per-wave snapshot lists (ranks through the commit directory
// only); directory mode: tdir levels instead of the first codes and no bucket
// table.  It depends on nt and ntiles alone, not on the instance launched.
struct LocLds {
    uint32_t first, cdir, hist, trad, sbuf, rbuf, bytes;
};
__host__ __device__ inline LocLds loc_lds(const NarrowTiles &nt, uint32_t ntiles)
{
    LocLds L{};
    uint32_t o = 0;
    L.first = o;
    o += 8 * (nt.trad ? ((ntiles + 1) & ~1u) : dir16_lds_entries(nt.tdir));
    L.cdir = o;
    o += nt.rank_lsn32 ? 0 : 8 * dir16_lds_entries(nt.cdir);
    L.hist = o;
    o += 4 * ((ntiles + 3) & ~3u);
    o = (o + 15) & ~15u;  // (the cdir levels are a multiple of 8 bytes only; the table is stored in 16-byte pieces)
    L.trad = o;
    o += nt.trad ? (uint32_t)narrow_trad16_bytes(nt.trad_m) : 0;
    // the snapshot lists serve the commit directory only; rbuf's first
    // kLocTThreads / 64 words hold the waves' totals of the tile scan in
    // every mode
    L.sbuf = o;
    o += nt.rank_lsn32 ? 0 : 8 * kLocTThreads;
    L.rbuf = o;
    o += 4 * (nt.rank_lsn32 ? kLocTThreads / 64 : kLocTThreads);
    L.bytes = o;
    return L;
}

// #first < x[k] over the LDS bucket table: bucket, then a binary search
// inside it (typically 0-1 steps; a crowded bucket costs log2 of its size).
// kMode: the table's mode when the instance fixes it (0 linear, 1 log), -1 =
// read from shift.
template <int K, int kMode = -1>
__device__ __forceinline__ void trad_count(const uint64_t *first, const uint16_t *T, uint32_t m,
                                           int shift, uint32_t ntiles, const uint64_t (&x)[K],
                                           const bool (&act)[K], uint32_t (&out)[K])
{
    uint32_t l[K], h[K];
    const bool lg = kMode < 0 ? (shift & kTradLog) != 0 : kMode == 1;
    const int sv = shift & 0xFFFF;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const uint64_t b = lg ? trad_log_bucket(x[k], sv) : x[k] >> sv;
        const bool in = b < m;
        const uint32_t bi = in ? (uint32_t)b : 0;
        l[k] = in ? T[bi] : ntiles;
        h[k] = in ? T[bi + 1] : ntiles;
    }
    for (;;) {
        bool more = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (l[k] < h[k]) {
                const uint32_t mid = (l[k] + h[k]) >> 1;
                const bool below = first[mid] < x[k];
                l[k] = below ? mid + 1 : l[k];
                h[k] = below ? h[k] : mid;
                more = true;
            }
        }
        if (!more) break;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = act[k] ? l[k] : 0;
}

// Whole-tile checks of a probe, deferred by one sub-chunk (their sparse-table
// loads then overlap the next sub-chunk's probe loads): tiles [x, y] hold a
// row committed after snap -> read set txn of probe q conflicts.
template <int K>
struct LocDefer {
    uint32_t x[K], y[K], q[K];
    uint64_t snap[K];
};

// work.vout[0 .. n_txn) and the bitmap's words := 0, workgroup g of work.G
// (kLocTThreads threads each): 16-byte pieces of the bytes between the
// buffer's first and last 16-byte boundary, the bytes outside them by
// workgroup 0's first threads.
__device__ __forceinline__ void zero_verdicts(const ProbeWork &work, uint32_t g)
{
    uint8_t *v = work.vout;
    const size_t nb = work.n_txn;
    const size_t head = std::min<size_t>(nb, (16 - ((uintptr_t)v & 15)) & 15);
    const size_t pieces = (nb - head) / 16, tail = head + 16 * pieces;
    const size_t t = (size_t)g * kLocTThreads + threadIdx.x, stride = (size_t)work.G * kLocTThreads;
    for (size_t i = t; i < pieces; i += stride) ((u32x4 *)(v + head))[i] = u32x4{0, 0, 0, 0};
    if (t < head) v[t] = 0;
    if (t < nb - tail) v[tail + t] = 0;
    if (work.bitmap)
        for (size_t i = t; i < ((size_t)work.n_txn + 63) / 64; i += stride) work.bitmap[i] = 0;
}

// W = key words held in registers (1 or 2), 0 = read from memory (any W).
// The chunk's kLocTP probes per thread run as kLocTP sub-chunks of one probe
// per thread: the loads of sub-chunk s + 1 are in flight while sub-chunk s is
// located (codes, snapshot ranks, end tiles, records), so the chunk's HBM
// reads overlap its LDS / VALU work instead of preceding it.  (r02,
// chunk-sorted records: 1 probe per sub-chunk 2.10 G vs 2 probes 2.00 G.)
//
// kShape: what the launch knows of the window and fixes for the instance.
// kLocGeneral reads everything from nv / nt at run time.  The fast shapes
// (kLocFastLin, kLocFastLog: W = 1 or 2 with the bucket table in linear / log
// mode) hold for a window without compressed codes whose last key word is its
// last varying limb (lw == W), with ranks in lsn32 mode, and a batch with
// probes (p.n > 0): no commit directory (its staging slots, snapshot lists
// and head search are not compiled), the bucket form a constant, bounds
// through locate_codes_fast.
constexpr int kLocGeneral = 0, kLocFastLin = 1, kLocFastLog = 2;
template <int W, bool kTrad, int kShape = kLocGeneral>
__global__ __launch_bounds__(kLocTThreads) void k_locate_t(NarrowView nv, WinView wt, ProbeView p,
                                                           ProbeWork work, NarrowTiles nt,
                                                           uint8_t *verdict)
{
    constexpr bool kFast = kShape != kLocGeneral;
    static_assert(!kFast || (kTrad && (W == 1 || W == 2)), "fast shapes: bucket table, 1 or 2 words");
    constexpr int WR = 2 > W ? 2 : W;
    constexpr int K = 1, S = kLocTP;  // probes per sub-chunk and thread, sub-chunks
    extern __shared__ __attribute__((aligned(16))) uint64_t lds64[];
    const uint32_t ntiles = wt.ntiles;
    const LocLds L = loc_lds(nt, ntiles);
    char *lb = (char *)lds64;
    uint64_t *tfirst = (uint64_t *)(lb + L.first);  // first codes (kTrad) / tdir levels
    uint64_t *cdir = (uint64_t *)(lb + L.cdir);
    uint32_t *hist = (uint32_t *)(lb + L.hist);
    uint16_t *T = (uint16_t *)(lb + L.trad);
    const int lane = threadIdx.x & 63;
    uint64_t *sb = (uint64_t *)(lb + L.sbuf) + (threadIdx.x & ~63u);
    uint32_t *rb = (uint32_t *)(lb + L.rbuf) + (threadIdx.x & ~63u);
    const uint32_t g = xcd_chunk(blockIdx.x, (work.G + 7) / 8);
    if (g >= work.G) return;
    HSC_STAMP(work, 0, 0);
    if (g == 0 && threadIdx.x < 3) work.item_off[threadIdx.x] = 0;  // the plan's / join's counters
    const uint32_t c0 = g * work.chunk;
    const uint32_t c1 = min(p.n, c0 + work.chunk);
    // probe registers: buffer 0 / 1 alternate between sub-chunks (the loop
    // below is unrolled, so every index is a compile-time constant)
    uint32_t qq[2][K], gg[2][K], tx[2][K];
    bool valid[2][K];
    uint64_t snap[2][K], xl[2][K][WR], xh[2][K][WR];
    // the chunk's records stay in registers until its histogram is complete,
    // then go to their tile-sorted places in the chunk's area
    uint4 R0[S][K], R1[S][K];
    uint32_t RT[S][K];
    uint64_t SS[S][K];  // ranks through the commit directory: the snapshots, ranked after the loop
    auto load = [&](int s, int buf) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int j = s * K + k;
            qq[buf][k] = c0 + threadIdx.x + kLocTThreads * j;
            valid[buf][k] = qq[buf][k] < c1;
            const uint32_t q = valid[buf][k] ? qq[buf][k] : 0;
            // read-once inputs: non-temporal, so they do not push the window's
            // rows out of the caches between batches
            // (a batch of table locks only has no probe arrays; the fast
            // shapes are launched with probes)
            const bool some = kFast || p.n;
            gg[buf][k] = some ? __builtin_nontemporal_load(p.gid + q) : 0;
            snap[buf][k] = some ? __builtin_nontemporal_load(p.snap + q) : 0;
            tx[buf][k] = some ? __builtin_nontemporal_load(p.txn + q) : 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                xl[buf][k][w] = some ? __builtin_nontemporal_load(p.lo + (size_t)w * p.n + q) : 0;
                xh[buf][k][w] = some ? __builtin_nontemporal_load(p.hi + (size_t)w * p.n + q) : 0;
            }
        }
    };
    load(0, 0);
    // Staging: every load is issued here, behind the first sub-chunk's probe
    // loads, into registers (the slot counts are compile-time, a slot past
    // the data reads piece 0 again: no branch around a load); the LDS stores
    // follow the histogram zeroing, so the phase costs one memory round trip
    // and not one per loop iteration.
    const int tshift = nt.trad_shift;
    u64x2 sf[kTradFirstSlots], st[kTradSlots];
    uint64_t sft = 0;  // an odd tile count's last first code
    u64x2 sd[kDirSlots], sc[kDirSlots];
    if constexpr (kTrad) {
        const u64x2 *src = (const u64x2 *)wt.sp_w;
        const u64x2 *src16 = (const u64x2 *)nt.trad16;
#pragma unroll
        for (int j = 0; j < kTradFirstSlots; ++j) {
            const uint32_t i = threadIdx.x + kLocTThreads * j;
            sf[j] = *(i < ntiles / 2 ? src + i : src16);  // (one tile: no whole piece of first codes)
        }
        sft = wt.sp_w[ntiles - 1];
#pragma unroll
        for (int j = 0; j < kTradSlots; ++j) {
            const uint32_t i = threadIdx.x + kLocTThreads * j;
            st[j] = src16[i < narrow_trad16_bytes(nt.trad_m) / 16 ? i : 0];
        }
    } else {
        dir16_stage_issue<kLocTThreads>(nt.tdir, sd);
    }
    const bool lsn32 = kFast || nt.rank_lsn32;
    if (!lsn32) dir16_stage_issue<kLocTThreads>(nt.cdir, sc);
    for (uint32_t i = threadIdx.x; i < ntiles; i += kLocTThreads) hist[i] = 0;
    if constexpr (kTrad) {
#pragma unroll
        for (int j = 0; j < kTradFirstSlots; ++j) {
            const uint32_t i = threadIdx.x + kLocTThreads * j;
            if (i < ntiles / 2) ((u64x2 *)tfirst)[i] = sf[j];
        }
        if ((ntiles & 1) && threadIdx.x == 0) tfirst[ntiles - 1] = sft;
#pragma unroll
        for (int j = 0; j < kTradSlots; ++j) {
            const uint32_t i = threadIdx.x + kLocTThreads * j;
            if (i < narrow_trad16_bytes(nt.trad_m) / 16) ((u64x2 *)T)[i] = st[j];
        }
    } else {
        dir16_stage_store<kLocTThreads>(nt.tdir, sd, tfirst);
    }
    if (!lsn32) dir16_stage_store<kLocTThreads>(nt.cdir, sc, cdir);
    __syncthreads();  // directories staged, histogram zeroed
    HSC_STAMP(work, 0, 1);
    const uint64_t *first = kTrad ? tfirst : wt.sp_w;  // first code of every tile
    // the fast shapes' base limbs and shift (uniform: scalar loads, once)
    uint64_t fbase[kFast ? W + 1 : 1] = {};
    const int ftz = nv.tz;
    if constexpr (kFast) {
#pragma unroll
        for (int i = 0; i <= W; ++i) fbase[i] = nv.base[i];
    }
    LocDefer<K> dfr;
#pragma unroll
    for (int k = 0; k < K; ++k) dfr.x[k] = 1, dfr.y[k] = 0;
    // A sub-chunk's candidate records get their in-chunk ranks here (fast
    // shapes; the general ones take them where the record is formed).  One LDS
    // word per tile: kept records in the low half (the returning add gives
    // the rank), located ones in the high half -- at most 4096 of a chunk
    // reach a tile, so no carry crosses.  A record the slot filter drops (sm:
    // the two slot maxima of each of the probe's records, ~0 = not tried)
    // adds to the located half only, without returning, and is gone.
    uint32_t sm[K][4];  // (not tried = 0xFFFFFFFF: no r(S) >> qshift is above it)
    auto commit = [&](int s) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint4 &a = R0[s][k], &b = R1[s][k];
            bool drop_a = false, drop_b = false;
            if constexpr (kFast) {
                const uint32_t qr = a.w >> nt.qshift;  // (both records carry the probe's r(S))
                drop_a = max(sm[k][0], sm[k][1]) < qr;
                drop_b = max(sm[k][2], sm[k][3]) < (b.w >> nt.qshift);
            }
            if (a.x != kNoTile32) {
                if (!drop_a)
                    a.x |= atomicAdd(&hist[a.x >> 12], 0x10001u) & 0xFFFFu;
                else
                    atomicAdd(&hist[a.x >> 12], 0x10000u), a.x = kNoTile32;
            }
            if (b.x != kNoTile32) {
                if (!drop_b)
                    b.x |= atomicAdd(&hist[b.x >> 12], 0x10001u) & 0xFFFFu;
                else
                    atomicAdd(&hist[b.x >> 12], 0x10000u), b.x = kNoTile32;
            }
        }
    };
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const int cb = s & 1;
        // 1. the previous sub-chunk's whole-tile checks: their loads are
        //    younger than this sub-chunk's probe loads, which are needed now;
        //    they are compared at the end of this sub-chunk (the loads
        //    overlap its LDS work; the read sets are in registers)
        uint64_t pm[K], psn[K];
        if (s > 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                pm[k] = dfr.x[k] <= dfr.y[k] ? tiles_max(wt, dfr.x[k], dfr.y[k]) : 0;
                psn[k] = dfr.snap[k];
            }
        }
        // 2. the next sub-chunk's probe loads stay in flight through step 3
        if (s + 1 < S) load(s + 1, cb ^ 1);
        // 3. locate this sub-chunk from registers and LDS
        uint64_t lo[K], hi[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if constexpr (kFast)
                locate_codes_fast<W>(ftz, fbase, valid[cb][k], gg[cb][k], xl[cb][k], xh[cb][k],
                                     lo[k], hi[k]);
            else
                locate_codes<W>(nv, p, valid[cb][k] ? qq[cb][k] : 0, gg[cb][k], xl[cb][k],
                                xh[cb][k], lo[k], hi[k]);
        }
        // Snapshot ranks r(S): O(1) when the window spans < 2^32 of log, else
        // #commits <= S through the commit directory; a run of equal
        // snapshots in neighbouring lanes (a read set's ranges) has one head,
        // the wave packs its heads into a list and searches each once.
        uint32_t rs[K];
        if (lsn32) {
#pragma unroll
            for (int k = 0; k < K; ++k) rs[k] = lsn32_rank(snap[cb][k], nt.rank_base);
        } else {
            // the records stay in registers: every sub-chunk's heads are
            // searched together after the loop (one directory walk, not S)
#pragma unroll
            for (int k = 0; k < K; ++k) rs[k] = 0, SS[s][k] = snap[cb][k];
        }
        // end tiles: a = #first < lo - 1 (the tile holding the first row >=
        // lo), bt = #first <= hi - 1 (the tile holding the last row <= hi)
        uint32_t cnt[2 * K];
        {
            uint64_t keys[2 * K];
            bool act[2 * K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                keys[2 * k] = lo[k];
                keys[2 * k + 1] = dir_le(hi[k]);
                act[2 * k] = act[2 * k + 1] = valid[cb][k] && lo[k] <= hi[k];
            }
            if constexpr (kTrad)
                trad_count<2 * K, kFast ? kShape == kLocFastLog : -1>(tfirst, T, nt.trad_m, tshift,
                                                                      ntiles, keys, act, cnt);
            else
                dir16_count<2 * K>(nt.tdir, tfirst, keys, act, cnt);
        }
        // the previous sub-chunk's records: its slot reads have had this
        // sub-chunk's codes and search to arrive
        if constexpr (kFast)
            if (s > 0) commit(s - 1);
        // records of the partly covered end tiles; the fully covered tiles
        // between them (and fully covered end tiles) become one deferred
        // range-maximum check [x, y]
#pragma unroll
        for (int k = 0; k < K; ++k) {
            dfr.x[k] = 1, dfr.y[k] = 0;
            R0[s][k].x = R1[s][k].x = kNoTile32;
            RT[s][k] = tx[cb][k];
            if constexpr (kFast) sm[k][0] = sm[k][1] = sm[k][2] = sm[k][3] = 0xFFFFFFFFu;
            if (!valid[cb][k]) continue;
            const uint32_t q = qq[cb][k];
            const uint32_t ca = cnt[2 * k], cbt = cnt[2 * k + 1];
            const uint32_t a = ca ? ca - 1 : 0;
            const uint32_t bt = cbt ? cbt - 1 : 0;
            uint4 r0 = make_uint4(kNoTile32, 0, 0, 0), r1 = r0;
            if (cbt > 0 && a <= bt && lo[k] <= hi[k]) {
                // tile-relative bounds
                const uint64_t fa = first[a], fb = first[bt];
                const uint64_t lo_a = lo[k] <= fa ? 0 : lo[k] - fa;  // > 2^32-1: none
                const uint64_t hi_a = a == bt ? (hi[k] < fa ? ~0ull : hi[k] - fa) : 0xFFFFFFFFull;
                const uint64_t hi_b = hi[k] < fb ? ~0ull : hi[k] - fb;
                const bool full_a = lo_a == 0 && (a < bt || hi_a >= 0xFFFFFFFFull);
                const bool use_a = lo_a <= 0xFFFFFFFFull && hi_a != ~0ull && lo_a <= hi_a;
                const bool use_b = a < bt && hi_b != ~0ull;
                const bool full_b = hi_b >= 0xFFFFFFFFull;
                dfr.x[k] = use_a && full_a ? a : a + 1;
                dfr.y[k] = a == bt ? (use_a && full_a ? a : 0) : (use_b && full_b ? bt : bt - 1);
                if (a == bt && !(use_a && full_a)) dfr.x[k] = 1, dfr.y[k] = 0;
                dfr.q[k] = q;
                dfr.snap[k] = snap[cb][k];
                const bool rec_a = use_a && !full_a, rec_b = use_b && !full_b;
                const uint32_t la = (uint32_t)lo_a, ha = (uint32_t)min(hi_a, 0xFFFFFFFFull);
                const uint32_t hb = (uint32_t)hi_b;
                if constexpr (kFast) {  // candidates: the in-chunk rank comes with commit()
                    if (rec_a) r0 = make_uint4(a << 12, la, ha, rs[k]);
                    if (rec_b) r1 = make_uint4(bt << 12, 0, hb, rs[k]);
                } else {  // the general shapes drop nothing: the word is a plain count
                    if (rec_a) r0 = make_uint4(a << 12 | atomicAdd(&hist[a], 1u), la, ha, rs[k]);
                    if (rec_b) r1 = make_uint4(bt << 12 | atomicAdd(&hist[bt], 1u), 0, hb, rs[k]);
                }
                // the slot filter (fast shapes): a record whose bounds reach at
                // most two adjacent slots of its tile, both with every row
                // older than the snapshot's quantum, meets no newer row.  Both
                // records' table reads go out here and are looked at one
                // sub-chunk later (commit), behind that one's end-tile search.
                if constexpr (kFast) {
                    const uint16_t *sa = nt.slots + (size_t)a * kSlots, *sb2 = nt.slots + (size_t)bt * kSlots;
                    const int sha = narrow_slot_shift(slot_span(tfirst, a, ntiles));
                    const int shb = narrow_slot_shift(slot_span(tfirst, bt, ntiles));
                    const uint32_t a0 = min(la >> sha, kSlots - 1), a1 = min(ha >> sha, kSlots - 1);
                    const uint32_t b1 = min(hb >> shb, kSlots - 1);
                    const bool try_a = rec_a && a1 - a0 <= 1, try_b = rec_b && b1 <= 1;
                    sm[k][0] = try_a ? sa[a0] : 0xFFFFFFFFu, sm[k][1] = try_a ? sa[a1] : 0xFFFFFFFFu;
                    sm[k][2] = try_b ? sb2[0] : 0xFFFFFFFFu, sm[k][3] = try_b ? sb2[b1] : 0xFFFFFFFFu;
                }
            }
            R0[s][k] = r0;
            R1[s][k] = r1;
        }
        if (s > 0) {  // step 1's compares (pm = 0 where there was no check)
#pragma unroll
            for (int k = 0; k < K; ++k)
                if (pm[k] > psn[k]) verdict[RT[s - 1][k]] = 1;
        }
    }
    // the last sub-chunk's range-maximum loads are issued here and compared
    // after the tail (scan, row and record stores), which they overlap
    uint64_t dmax[K];
#pragma unroll
    for (int k = 0; k < K; ++k) dmax[k] = dfr.x[k] <= dfr.y[k] ? tiles_max(wt, dfr.x[k], dfr.y[k]) : 0;
    if constexpr (kFast) commit(S - 1);
    {
        if (!lsn32) {  // the chunk's snapshot ranks: heads of all sub-chunks in one list
            const uint64_t le_mask = lane == 63 ? ~0ull : ((2ull << lane) - 1);
            bool head[S][K];
            uint32_t slot[S][K];
            uint32_t H = 0;
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const uint64_t prev = __shfl_up(SS[s][k], 1, 64);
                    head[s][k] = lane == 0 || prev != SS[s][k];
                    const uint64_t m = __ballot(head[s][k]);
                    slot[s][k] = H + __popcll(m & le_mask) - 1;  // this lane's head
                    H += __popcll(m);
                }
            for (uint32_t b0 = 0; b0 < H; b0 += 64) {
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (head[s][k] && slot[s][k] - b0 < 64) sb[slot[s][k] - b0] = SS[s][k];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const bool act[1] = {lane < H - b0};
                const uint64_t xs[1] = {act[0] ? dir_le(sb[lane]) : 0};
                uint32_t r[1];
                dir16_count<1>(nt.cdir, cdir, xs, act, r);
                rb[lane] = r[0];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int k = 0; k < K; ++k)
                        if (slot[s][k] - b0 < 64) R0[s][k].w = R1[s][k].w = rb[slot[s][k] - b0];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
    }
    HSC_STAMP(work, 0, 2);
    // table locks: any write to a locked table after the snapshot
    for (uint32_t q = g * kLocTThreads + threadIdx.x; q < p.n_lock; q += work.G * kLocTThreads) {
        const uint32_t t = p.lock_table[q];
        if (t < wt.ntables && wt.table_max[t] > p.lock_snap[q]) verdict[p.lock_txn[q]] = 1;
    }
    __syncthreads();
    HSC_STAMP(work, 0, 3);
    // column g of the tile-major histogram (neighbouring chunks of a line are
    // written from the same XCD)
    {
        // exclusive scan of the chunk's tile counts (thread = a run of
        // consecutive tiles): row g of the chunk-major table gets (run start
        // << 16 | count) per tile (contiguous stores; the plan transposes),
        // the runs' starts replace the counts in LDS
        const uint32_t per = (ntiles + kLocTThreads - 1) / kLocTThreads;
        const uint32_t i0 = min(ntiles, threadIdx.x * per), i1 = min(ntiles, i0 + per);
        uint32_t sum = 0;
        constexpr uint32_t kCount = kFast ? 0xFFFFu : 0xFFFFFFFFu;  // (a general shape's word is the count)
        for (uint32_t i = i0; i < i1; ++i) sum += hist[i] & kCount;
        uint32_t x = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        uint32_t *wtot = (uint32_t *)(lb + L.rbuf);
        if (lane == 63) wtot[threadIdx.x >> 6] = x;
        __syncthreads();
        uint32_t run = x - sum;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); ++w) run += wtot[w];
        // (the fast shapes write two-word entries: the general ones drop
        // nothing, located = kept, and keep the one-word table)
        const size_t ro = (size_t)g * ((ntiles + 3) & ~3u);
        for (uint32_t i = i0; i < i1; ++i) {
            const uint32_t h = hist[i], c = h & kCount;
            if constexpr (kFast)
                work.cmx[ro + i] = make_uint2(run << 16 | c, h >> 16);  // (located, before the filter)
            else
                work.cm[ro + i] = run << 16 | c;
            hist[i] = run;
            run += c;
        }
        __syncthreads();
        HSC_STAMP(work, 0, 4);
        uint4 *area = nt.recs + (size_t)g * 2 * work.chunk;
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint4 a = R0[s][k], b = R1[s][k];
                if (a.x != kNoTile32)
                    area[hist[a.x >> 12] + (a.x & 0xFFFu)] = make_uint4(a.y, a.z, a.w, RT[s][k]);
                if (b.x != kNoTile32)
                    area[hist[b.x >> 12] + (b.x & 0xFFFu)] = make_uint4(b.y, b.z, b.w, RT[s][k]);
            }
        // no plan after this locate: chunk g's workgroup clears its slice of
        // the caller's verdict bytes and bitmap words (no kernel marks them
        // before the join).  Issued here, behind the record stores: nothing
        // in the kernel waits for them (in the prologue the first workgroups'
        // next probe loads waited for their acknowledgements, +0.9 us on
        // config 2's one wave of workgroups)
        if (work.vout) zero_verdicts(work, g);
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (dfr.x[k] <= dfr.y[k] && dmax[k] > dfr.snap[k]) verdict[RT[S - 1][k]] = 1;
    }
    HSC_STAMP(work, 0, 5);
}

// The window's shape: the fast instances are built for a batch with probes
// over a bucket-table window of 1 or 2 words, no compressed codes, the last
// word the last varying limb, ranks in lsn32 mode (W = 1 with a log table has
// no instance: it takes the general one).
bool narrow_locate_fast(const NarrowView &nv, const NarrowTiles &nt, const ProbeView &p)
{
    const int w = nv.W == 1 || nv.W == 2 ? nv.W : 0;
    const bool tr = nt.trad != nullptr;
    const bool log = tr && (nt.trad_shift & (int)kTradLog) != 0;
    return tr && w != 0 && !nv.comp && nv.lw == nv.W && nt.rank_lsn32 && p.n > 0 && !(log && w == 1);
}

hipError_t launch_locate_t(const NarrowView &nv, const WinView &wt, const ProbeView &p,
                           const ProbeWork &work, const NarrowTiles &nt, uint8_t *verdict,
                           hipStream_t s, int *shape)
{
    if (shape) *shape = -1;
    if (p.n == 0 && p.n_lock == 0) return hipSuccess;
    const size_t lds = loc_lds(nt, wt.ntiles).bytes;
    const bool tr = nt.trad != nullptr;
    // what the kernel's staging slots hold
    if (tr ? wt.ntiles > kTradMaxTiles || nt.trad_m > kTradMax || !nt.trad16
           : nt.tdir.lds_n > (uint32_t)kDirLds)
        return hipErrorInvalidValue;
    if (!nt.rank_lsn32 && nt.cdir.lds_n > (uint32_t)kDirLds) return hipErrorInvalidValue;
    const int w = nv.W == 1 || nv.W == 2 ? nv.W : 0;
    const bool log = tr && (nt.trad_shift & (int)kTradLog) != 0;
    const bool fast = narrow_locate_fast(nv, nt, p);
    // the table's layout is the caller's choice by the same rule: two-word
    // entries (cmx) for a fast instance, one-word entries (cm) otherwise
    if (fast ? !work.cmx || work.cm : !work.cm || work.cmx) return hipErrorInvalidValue;
    if (shape) *shape = fast ? 1 : 0;
#define HSC_LOCATE(W_, TR_, ...)                                                                  \
    k_locate_t<W_, TR_, ##__VA_ARGS__><<<8 * ((work.G + 7) / 8), kLocTThreads, lds, s>>>(nv, wt, p, work, \
                                                                                   nt, verdict)
    if (fast && w == 1)
        HSC_LOCATE(1, true, kLocFastLin);
    else if (fast && !log)
        HSC_LOCATE(2, true, kLocFastLin);
    else if (fast)
        HSC_LOCATE(2, true, kLocFastLog);
    else if (w == 1 && tr)
        HSC_LOCATE(1, true);
    else if (w == 1)
        HSC_LOCATE(1, false);
    else if (w == 2 && tr)
        HSC_LOCATE(2, true);
    else if (w == 2)
        HSC_LOCATE(2, false);
    else if (tr)
        HSC_LOCATE(0, true);
    else
        HSC_LOCATE(0, false);
#undef HSC_LOCATE
    return hipGetLastError();
}

// probes per locate workgroup, directory entries staged in LDS
uint32_t narrow_tiles_chunk() { return kLocTP * kLocTThreads; }
uint32_t narrow_tiles_dir_lds() { return kDirLds; }

// A tile that the locate's end-tile step gave more than kTileCap records --
// located records, counted before the slot filter drops any (ProbeWork::cmx) --
// tells the host (ProbeWork::hot): every such tile of a batch stores the same
// value, written through to host memory.  The rounds and overflow items that
// run are sized by the records the filter kept.
__device__ __forceinline__ void mark_hot(const ProbeWork &work)
{
    if (work.hot) __hip_atomic_store(work.hot, work.batch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- plan ----
// ctl[1] (extra join items) was zeroed by this batch's locate.
// Plan of chunk-sorted records: block = 8 tiles (kPlanSThreads / 64).
// The block reads the tiles' entries of every chunk row of the locate's
// chunk-major table (32 contiguous bytes per row), transposes them through LDS, and wave w scans
// tile t0 + w's column as k_plan_t does; it writes the tile-major exclusive
// offsets (hist) and run starts (cst) the join stages, the tile's count and,
// for a hot tile, join items over its own record numbers.  The verdict pack
// is folded in as in k_plan_t.
// 512 threads (8 tiles, 32-byte row pieces) vs 1024 (16 tiles, 64-byte
// pieces): one stream 62.1 vs 61.1 us, two streams 2.22 vs 2.17 G checks/s
// (r02d) -- the headline is the two-stream number
constexpr int kPlanSThreads = 512;  // a wave per tile
// kWide: the table has two-word entries (work.cmx, a fast narrow locate);
// else one-word entries (work.cm), located = kept, and no LDS for a second count
template <bool kWide>
__global__ __launch_bounds__(kPlanSThreads) void k_plan_s(ProbeWork work, uint32_t ntiles,
                                                          uint32_t *ctl, uint8_t *flags,
                                                          uint32_t n_txn, uint8_t *verdict)
{
    constexpr int TB = kPlanSThreads / 64;  // tiles per block
    static_assert(TB % 4 == 0, "16-byte row pieces");
    constexpr uint32_t SR = kMaxChunks + 4;
    __shared__ __attribute__((aligned(16))) uint32_t sh[TB][SR];
    __shared__ uint16_t shl[kWide ? TB : 1][kWide ? SR : 1];  // the located counts of the same entries
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t t0 = blockIdx.x * TB, t = t0 + w;
    const uint32_t G = work.G, hs = hist_stride(G), rs = (ntiles + 3) & ~3u;
    // (g, piece) pairs: TB / 4 16-byte pieces of every chunk row
    for (uint32_t i = threadIdx.x; i < G * (TB / 4); i += kPlanSThreads) {
        const uint32_t g = i / (TB / 4), pc = i % (TB / 4);
        const uint32_t c = t0 + 4 * pc;
        if constexpr (kWide) {  // two-word entries: 32 bytes per piece
            const u32x4 *src = (const u32x4 *)(work.cmx + (size_t)g * rs + c);
            const u32x4 z = {0, 0, 0, 0};
            const u32x4 a = c < rs ? src[0] : z, b = c < rs ? src[1] : z;
            sh[4 * pc][g] = a.x, sh[4 * pc + 1][g] = a.z, sh[4 * pc + 2][g] = b.x, sh[4 * pc + 3][g] = b.z;
            shl[4 * pc][g] = (uint16_t)a.y, shl[4 * pc + 1][g] = (uint16_t)a.w;
            shl[4 * pc + 2][g] = (uint16_t)b.y, shl[4 * pc + 3][g] = (uint16_t)b.w;
        } else {
            const u32x4 a = c < rs ? *(const u32x4 *)(work.cm + (size_t)g * rs + c) : u32x4{0, 0, 0, 0};
            sh[4 * pc][g] = a.x, sh[4 * pc + 1][g] = a.y, sh[4 * pc + 2][g] = a.z, sh[4 * pc + 3][g] = a.w;
        }
    }
    if (verdict) {
        // (a wave covers 64 consecutive read sets, 64-aligned: one bitmap word)
        const uint32_t stride = gridDim.x * kPlanSThreads;
        for (uint32_t i = blockIdx.x * kPlanSThreads + threadIdx.x; i < n_txn; i += stride) {
            const uint8_t f = flags[i];
            verdict[i] = f != 0;
            if (f) flags[i] = 0;
            const uint64_t m = __ballot(f != 0);
            if (work.bitmap && lane == 0) work.bitmap[i >> 6] = m;
        }
    }
    __syncthreads();
    if (t >= ntiles) return;
    const uint32_t e = 8 * lane;
    uint32_t v[8], c[8], located = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t x = e + k < G ? sh[w][e + k] : 0;
        v[k] = x & 0xFFFFu;
        c[k] = x >> 16;
        if constexpr (kWide) located += e + k < G ? shl[w][e + k] : 0;
    }
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) sum += v[k];
    uint32_t x = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    uint32_t run = x - sum;
    if (e < hs) {
        u32x4 oa, ob;
        oa.x = run; run += v[0];
        oa.y = run; run += v[1];
        oa.z = run; run += v[2];
        oa.w = run; run += v[3];
        ob.x = run; run += v[4];
        ob.y = run; run += v[5];
        ob.z = run; run += v[6];
        ob.w = run;
        u32x4 *col = (u32x4 *)(work.hist + (size_t)t * hs);
        col[e / 4] = oa;
        col[e / 4 + 1] = ob;
        *(u32x4 *)(work.cst + (size_t)t * hs + e) =
            u32x4{c[0] | c[1] << 16, c[2] | c[3] << 16, c[4] | c[5] << 16, c[6] | c[7] << 16};
    }
    const uint32_t total = __shfl(x, 63, 64);
    if (lane == 0) work.counts[t] = total;
    // the hot rule: located records (the tile's total where nothing is dropped)
    if constexpr (kWide) {
#pragma unroll
        for (int o = 32; o; o >>= 1) located += __shfl_xor(located, o, 64);
    } else {
        located = total;
    }
    if (lane == 0 && located > kTileCap) mark_hot(work);
    if (total > kTileCap) {  // join items over the kept records past kTileCap
        const uint32_t over = total - kTileCap;
        const uint32_t nx = (over + kJoinChunk - 1) / kJoinChunk;
        uint32_t ib = 0;
        if (lane == 0) ib = atomicAdd(&ctl[1], nx);
        ib = __shfl(ib, 0, 64);
        for (uint32_t j = lane; j < nx; j += 64)
            work.item_desc[ib + j] = make_uint4(t, kTileCap + j * kJoinChunk,
                                                kTileCap + min((j + 1) * kJoinChunk, over), 0);
    }
}

hipError_t launch_plan_s(const ProbeWork &work, uint32_t ntiles, uint32_t *ctl, hipStream_t s,
                         uint8_t *flags, uint32_t n_txn, uint8_t *verdict)
{
    if (ntiles == 0) return hipSuccess;
    constexpr uint32_t per = kPlanSThreads / 64;
    if (work.cmx)
        k_plan_s<true><<<(ntiles + per - 1) / per, kPlanSThreads, 0, s>>>(work, ntiles, ctl, flags, n_txn,
                                                                          verdict);
    else
        k_plan_s<false><<<(ntiles + per - 1) / per, kPlanSThreads, 0, s>>>(work, ntiles, ctl, flags, n_txn,
                                                                           verdict);
    return hipGetLastError();
}

// ---- join: 8-byte rows ----
// A block stages its tile's recent list (wave 0: a quad of keys, already in
// Eytzinger order, and one of ranks per lane) and only for old snapshots the
// whole tile (below) -- row quad v of thread t = rows 4 (t + kJoinThreads v)
// .. + 3: one 16-byte load of keys (k_key32's order) and one of ranks per
// quad.  Either way the quads are stored to LDS as they are, with 16-row
// maxima over 4 lanes and 128-row maxima over 32 lanes.

// The join is held to 8 waves per SIMD: at 85-99 SGPRs the hardware admits
// only 6-7 (measured on config 2: join 34 -> 31.7 us, one stream 71.3 -> 69 us)
// Chunk-sorted records: record j of tile t lives in the
// run of the chunk g whose offset inside the tile (the plan's scan of column
// t) is the last one <= j, at chunk g's area + cst[t][g] + (j - that offset).
// The tile's column is staged first (its loads ahead of the list's), each
// thread finds its records' chunks by a 9-step search of it in LDS and issues
// the record loads.
// kJoinCol (no plan ran): the block reads column `tile` of the locate's
// chunk-major table itself -- thread g the entry of chunk g, 4-byte loads that
// the tiles sharing a line of a chunk row (neighbours on one XCD) find in its
// L2 after the first touch (the table in pieces of 4 tiles, a column 16 bytes
// apart, measured the same: 41.3 vs 41.5 us per two-stream step, within the
// spread) -- and scans the counts over its 8 waves: Es, Cs, the tile's total.
// It runs every record of the tile, kJoinChunk a round; the list, the column
// and (once a round needs it) the tile's rows are staged once and only read
// afterwards.
enum JoinMode { kJoinItem, kJoinTile, kJoinCol };

// Read set i's flag of the locate into its verdict byte and bitmap bit; set
// flags are cleared for the next batch.  Only ones are written, so the move
// commutes with the hits other blocks mark.  Whole waves call it (f = 0 past
// n_txn): a wave's 64 read sets share one bitmap word.
__device__ __forceinline__ void move_flag(const ProbeWork &work, uint8_t *flags, uint8_t *verdict,
                                          uint32_t i, uint8_t f)
{
    if (f) verdict[i] = 1, flags[i] = 0;
    if (work.bitmap) {
        const uint64_t m = __ballot(f != 0);
        if (m && (threadIdx.x & 63) == 0) atomicOr((unsigned long long *)&work.bitmap[i >> 6], m);
    }
}

// The strides of a block's share past the first (a batch of more read sets
// than the grid has threads): four loads in flight.
__device__ __forceinline__ void move_flags_rest(const ProbeWork &work, uint8_t *flags, uint8_t *verdict,
                                                uint32_t fi, uint32_t fstride)
{
    for (size_t i = (size_t)fi + fstride; i < work.n_txn; i += 4 * (size_t)fstride) {
        uint8_t f[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) f[k] = i + (size_t)k * fstride < work.n_txn ? flags[i + (size_t)k * fstride] : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) move_flag(work, flags, verdict, (uint32_t)(i + (size_t)k * fstride), f[k]);
    }
}

// The rows a join block stages.  Exactness rule of the recent list (k_recent):
// if r(S) >= rtheta[t], every row of tile t with rank32 > r(S) is a list
// member -- a row left out has rank32 <= rtheta[t] <= r(S), ties included --
// so "some member has lo <= key <= hi and rank32 > r(S)" is the whole tile's
// answer.  A block therefore stages the tile's list (2 KB) and walks its
// records over it, 8 levels instead of 12, as long as every live record of
// the round has r(S) >= rtheta[t]: one block-wide vote per round.  The first
// round that fails the vote stages the whole tile (32 KB, into
// arrays of its own, so the list's readers need no barrier), counts itself in
// work.full_joins, and the tile stays staged for the item's remaining rounds.
struct JoinLds {
    uint32_t *keys, *rank, *b16, *b128;      // the whole tile
    uint32_t *lkeys, *lrank, *lb16, *lb128;  // its recent list
    uint32_t *Es, *Cs, *vote;  // vote[2]: a round's "stage the whole tile"
};

// kMove (kJoinCol): the block moves its share of the locate's flags here;
// k_join_w's blocks have moved theirs before they call this for a tile
template <JoinMode kMode, bool kMove = true>
__device__ __forceinline__ void join_s_item(const ProbeWork &work, const NarrowTiles &nt,
                                            uint32_t n, uint32_t xi, uint8_t *verdict,
                                            const JoinLds &L,
                                            uint32_t rs = 0, uint8_t *flags = nullptr,
                                            uint32_t *wtot = nullptr)
{
    constexpr uint32_t T = 1u << kTLog2;
    constexpr int RQ = T / (4 * kJoinThreads);
    constexpr int kRec = kJoinChunk / kJoinThreads;
    static_assert(kMaxChunks <= kJoinThreads, "one column entry per thread");
    uint32_t *const Es = L.Es, *const Cs = L.Cs;
    uint32_t tile, j0, j1;
    if constexpr (kMode != kJoinItem) {
        tile = xi, j0 = 0;
    } else {
        const uint32_t *d = (const uint32_t *)(work.item_desc + xi);
        tile = sload(d), j0 = sload(d + 1), j1 = sload(d + 2);
    }
    const uint32_t G = work.G;
    uint32_t e = 0, cs = 0, el = 0;  // el: chunk g's located records of the tile
    // this block's share of the flags: the first stride's load goes out ahead
    // of the column's and the list's
    const uint32_t fstride = gridDim.x * kJoinThreads, fi = blockIdx.x * kJoinThreads + threadIdx.x;
    uint8_t f0 = 0;
    if constexpr (kMode == kJoinCol) {
        if (kMove && fi < work.n_txn) f0 = flags[fi];
        if (threadIdx.x < G) {
            if (work.cmx) {  // one 8-byte load: both words of the entry
                const uint2 ex = work.cmx[(size_t)threadIdx.x * rs + tile];
                e = ex.x, el = ex.y;
            } else {  // a general locate: located = kept
                e = work.cm[(size_t)threadIdx.x * rs + tile];
                el = e & 0xFFFFu;
            }
        }
    } else {
        const size_t col = (size_t)tile * hist_stride(G);
        if (threadIdx.x < G) {
            e = work.hist[col + threadIdx.x];
            cs = work.cst[col + threadIdx.x];
        }
    }
    // the tile's list: wave 0, a quad of keys and one of ranks per lane
    const uint32_t theta = sload(nt.rtheta + tile);
    u32x4 lk = {0, 0, 0, 0}, lr = {0, 0, 0, 0};
    if (threadIdx.x < kRecent / 4) {
        const size_t q = (size_t)tile * kRecent + 4 * threadIdx.x;
        lk = *(const u32x4 *)(nt.rkey32 + q);
        lr = *(const u32x4 *)(nt.rrank32 + q);
    }
    u32x4 rec[kRec];
    if constexpr (kMode == kJoinCol) {
        if constexpr (kMove) {
            move_flag(work, flags, verdict, fi, f0);
            move_flags_rest(work, flags, verdict, fi, fstride);
        }
        // block-exclusive scan of the column's counts: wave scans, then the
        // 8 wave totals through LDS
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint32_t cnt = e & 0xFFFFu;
        uint32_t x = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wtot[wave] = x;
        __syncthreads();
        uint32_t run = x - cnt, total = 0;
#pragma unroll
        for (int w = 0; w < kJoinThreads / 64; ++w) {
            const uint32_t t = wtot[w];
            run += w < wave ? t : 0;
            total += t;
        }
        cs = e >> 16, e = run;
        j1 = __builtin_amdgcn_readfirstlane(total);
        if (threadIdx.x == 0) work.counts[tile] = j1;  // (read back by the timing statistics)
    }
    if constexpr (kMode == kJoinTile) j1 = min(kTileCap, sload(work.counts + tile));
    if (kMode == kJoinCol || threadIdx.x < G) Es[threadIdx.x] = e, Cs[threadIdx.x] = cs;
    // a quad's ranks into 16-row maxima (4 lanes) and 128-row maxima (32 lanes)
    auto maxima = [](const u32x4 &r, uint32_t quad, uint32_t *b16, uint32_t *b128) {
        uint32_t m = max(max(r.x, r.y), max(r.z, r.w));
        m = max(m, (uint32_t)__shfl_xor((int)m, 1, 64));
        m = max(m, (uint32_t)__shfl_xor((int)m, 2, 64));
        if ((threadIdx.x & 3) == 0) b16[quad >> 2] = m;
#pragma unroll
        for (int d = 4; d < 32; d <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
        if ((threadIdx.x & 31) == 0) b128[quad >> 5] = m;
    };
    if (threadIdx.x < kRecent / 4) {  // (wave 0 as a whole)
        ((u32x4 *)L.lkeys)[threadIdx.x] = lk;
        ((u32x4 *)L.lrank)[threadIdx.x] = lr;
        maxima(lr, threadIdx.x, L.lb16, L.lb128);
        if (threadIdx.x < 2) L.vote[threadIdx.x] = 0;
    }
    // the hot rule counts located records: their sum needs no scan and rides
    // the list's barrier -- a second word per wave, read by thread 0 behind it
    if constexpr (kMode == kJoinCol) {
#pragma unroll
        for (int o = 32; o; o >>= 1) el += __shfl_xor(el, o, 64);
        if ((threadIdx.x & 63) == 0) wtot[kJoinThreads / 64 + (threadIdx.x >> 6)] = el;
    }
    __syncthreads();
    if constexpr (kMode == kJoinCol) {
        if (threadIdx.x == 0) {
            uint32_t located = 0;
#pragma unroll
            for (int w = 0; w < kJoinThreads / 64; ++w) located += wtot[kJoinThreads / 64 + w];
            if (located > kTileCap) mark_hot(work);
        }
    }
    HSC_STAMP(work, 1, 1);
    const size_t area = 2 * (size_t)work.chunk;
    // Record slot k of this thread in the round at jb (kNoRec: none).  A round
    // of more than kJoinThreads records maps slot k to record jb + k *
    // kJoinThreads + thread.  A smaller one -- what the locate's filter leaves
    // of most tiles -- is dealt out as equal runs of consecutive records
    // (eight of them from 128 records on, runs of kDealMin below), one per
    // wave in slot 0 -- on the column path only (kJoinCol): the plan path's
    // tile blocks and overflow items keep the thread-order mapping, which is
    // what config 5's 33-record tiles ran faster with: in thread order its few records would
    // all sit in wave 0, whose range-maximum passes the other seven waves
    // would wait for at the barrier.  skip (wave-uniform): the wave's run of
    // this slot is empty.
    constexpr uint32_t kNoRec = 0xFFFFFFFFu;
    // a wave's run is never shorter than 16 records while there are that many:
    // wave_any_after32 resolves one range per 16-lane group and pass, so runs
    // below 16 only add waves that walk (measured on config 2, two streams:
    // 37.7-38.0 us with eight runs always, 36.8-37.1 with this floor)
    constexpr uint32_t kDealMin = 16;
    auto slot = [&](uint32_t jb, int k, bool &skip) -> uint32_t {
        const uint32_t m = j1 > jb ? min(j1 - jb, (uint32_t)kJoinChunk) : 0;  // block-uniform
        if (kMode == kJoinCol && m <= (uint32_t)kJoinThreads) {
            const uint32_t per = max((m + kJoinThreads / 64 - 1) / (kJoinThreads / 64), kDealMin);  // <= 64
            const uint32_t w0 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) * per;
            const uint32_t lane = threadIdx.x & 63;
            skip = k > 0 || w0 >= m;
            return !skip && lane < per && w0 + lane < m ? jb + w0 + lane : kNoRec;
        }
        const uint32_t j = jb + k * kJoinThreads + threadIdx.x;
        skip = __builtin_amdgcn_readfirstlane(j) >= j1;
        return j < j1 ? j : kNoRec;
    };
    // a round's record loads: records jb .. jb + kJoinChunk of the tile
    auto fetch = [&](uint32_t jb) {
#pragma unroll
        for (int k = 0; k < kRec; ++k) {
            bool skip;
            const uint32_t j = slot(jb, k, skip);
            // a wave with no record in this slot has nothing to search or load
            // (walk skips it the same way; the vote reads its records as empty)
            if (skip) {
                rec[k] = u32x4{0, 0, 0, 0};
                continue;
            }
            uint32_t g = 0;  // Es[0] = 0 <= j
#pragma unroll
            for (int b = 8; b >= 0; --b) {
                const uint32_t c = g + (1u << b);
                if (c < G && Es[c] <= j) g = c;
            }
            rec[k] = j != kNoRec ? *(const u32x4 *)(nt.recs + g * area + Cs[g] + (j - Es[g]))
                                 : u32x4{0, 0, 0, 0};
        }
    };
    // the whole tile: rows and maxima to LDS as they lie (today's staging)
    auto stage_tile = [&]() {
        u32x4 rk[RQ], rr[RQ];
        const size_t ts = (size_t)tile << kTLog2;
#pragma unroll
        for (int v = 0; v < RQ; ++v) {
            const size_t row = ts + 4 * (threadIdx.x + kJoinThreads * v);
            rk[v] = *(const u32x4 *)(nt.key32 + row);
            rr[v] = *(const u32x4 *)(nt.rank32 + row);
        }
#pragma unroll
        for (int v = 0; v < RQ; ++v) {
            const uint32_t quad = threadIdx.x + kJoinThreads * v;
            ((u32x4 *)L.keys)[quad] = rk[v];
            ((u32x4 *)L.rank)[quad] = rr[v];
            maxima(rr[v], quad, L.b16, L.b128);
        }
        if (threadIdx.x == 0 && work.full_joins) atomicAdd(work.full_joins, 1u);
        __syncthreads();
    };
    const uint32_t tn = min(T, n - (tile << kTLog2));
    // records r0 .. of the round over a sorted run of nrow rows staged as a
    // 2^LV-entry Eytzinger tree (keys), ranks in row order and their maxima
    auto walk = [&](uint32_t r0, auto lv, const uint32_t *keys, const uint32_t *rank,
                    const uint32_t *b16, const uint32_t *b128, uint32_t nrow) {
        constexpr int LV = decltype(lv)::value;
        constexpr uint32_t N = 1u << LV;
#pragma unroll
        for (int k = 0; k < kRec; ++k) {
            bool skip;
            const uint32_t j = slot(r0, k, skip);
            // a wave with no record in this slot skips it as a whole; inside, a
            // lane's record is a predicate (the range maxima are resolved by the wave)
            if (skip) continue;
            const uint32_t lo = rec[k].x, hi = rec[k].y, rs = rec[k].z;
            uint32_t ja = 1, jb = 1;
#pragma unroll
            for (int d = 0; d < LV; ++d) {
                const uint32_t ka = keys[ja], kb = keys[jb];
                ja = 2 * ja + (ka < lo);
                jb = 2 * jb + (kb <= hi);
            }
            const uint32_t kl = keys[0];
            const uint32_t pa = min(ja - N + (kl < lo), nrow);
            const uint32_t pb = min(jb - N + (kl <= hi), nrow);
            if (wave_any_after32(rank, b16, b128, pa, pb, rs, j != kNoRec && pa < pb)) {
                // (r05w, world-1 per-rank step: these atomics 50.7 / 51.9 us per
                // step, guarded by a read of the verdict byte 53.3 / 52.5, the
                // pack pass instead 52.7 / 51.9 -- the same within the spread)
                verdict[rec[k].w] = 1;
                if (work.bitmap)
                    atomicOr((unsigned long long *)&work.bitmap[rec[k].w >> 6], 1ull << (rec[k].w & 63));
            }
        }
    };
    bool full = false;  // block-uniform: the whole tile is staged
    auto round = [&](uint32_t jb) {
        fetch(jb);
        if (!full) {
            // a live record whose snapshot is older than a row left out of the list?
            bool old = false;
#pragma unroll
            for (int k = 0; k < kRec; ++k) {
                bool skip;
                old |= slot(jb, k, skip) != kNoRec && rec[k].x <= rec[k].y && rec[k].z < theta;
            }
            // (a slot per round parity: a wave already in the next round's vote
            // must not change what a slower wave still has to read of this one's)
            uint32_t *vote = L.vote + (jb / kJoinChunk & 1);
            if (__ballot(old) && (threadIdx.x & 63) == 0) *vote = 1;
            __syncthreads();
            full = __builtin_amdgcn_readfirstlane(*vote) != 0;
            if (full) stage_tile();
        }
        if (jb == j0) HSC_STAMP(work, 1, 2);
        if (full)
            walk(jb, std::integral_constant<int, kTLog2>{}, L.keys, L.rank, L.b16, L.b128, tn);
        else
            walk(jb, std::integral_constant<int, kRecentLog2>{}, L.lkeys, L.lrank, L.lb16, L.lb128,
                 min(kRecent, tn));
    };
    round(j0);
    if constexpr (kMode == kJoinCol) {  // a hot tile: the rounds past the first
        for (uint32_t jb = kJoinChunk; jb < j1; jb += kJoinChunk) round(jb);
    }
}

// the tiles' blocks, a multiple of 8: tile = xcd_chunk(block) (r02c: config 2
// 2.09 -> 2.16 G checks/s, join 31.7 -> 29.6 us against tile = block)
__host__ __device__ inline uint32_t join_tile_blocks(uint32_t ntiles) { return 8 * ((ntiles + 7) / 8); }

// kCol: no plan ran (launch_join_col) -- a block per tile and nothing else;
// the blocks past the tiles (the grid is a multiple of 8) still move their
// share of the flags.
template <bool kCol>
__global__ __launch_bounds__(kJoinThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_join_t(
    ProbeWork work, NarrowTiles nt, uint32_t n, uint32_t ntiles, uint8_t *verdict, uint8_t *flags)
{
    constexpr uint32_t T = 1u << kTLog2;
    __shared__ __attribute__((aligned(16))) uint32_t keys[T];
    __shared__ __attribute__((aligned(16))) uint32_t rank[T];
    __shared__ uint32_t b16[T / 16];
    __shared__ uint32_t b128[T / 128];
    __shared__ __attribute__((aligned(16))) uint32_t lkeys[kRecent];
    __shared__ __attribute__((aligned(16))) uint32_t lrank[kRecent];
    __shared__ uint32_t lb16[kRecent / 16], lb128[kRecent / 128];
    __shared__ uint32_t Es[kMaxChunks], Cs[kMaxChunks], vote[2];
    const JoinLds L{keys, rank, b16, b128, lkeys, lrank, lb16, lb128, Es, Cs, vote};

    HSC_STAMP(work, 1, 0);
    // chunk-sorted records: neighbouring tiles on one XCD (their runs of a
    // chunk share lines of its record area, which that XCD's L2 then serves)
    const uint32_t tb = join_tile_blocks(ntiles);
    if constexpr (kCol) {
        __shared__ uint32_t wtot[2 * (kJoinThreads / 64)];  // kept and located, per wave
        const uint32_t tile = xcd_chunk(blockIdx.x, tb / 8);
        if (tile < ntiles) {
            join_s_item<kJoinCol>(work, nt, n, tile, verdict, L,
                                  (ntiles + 3) & ~3u, flags, wtot);
        } else {
            for (uint32_t i = blockIdx.x * kJoinThreads + threadIdx.x; i < work.n_txn;
                 i += gridDim.x * kJoinThreads)
                move_flag(work, flags, verdict, i, flags[i]);
        }
    } else if (blockIdx.x < tb) {
        const uint32_t tile = xcd_chunk(blockIdx.x, tb / 8);
        if (tile < ntiles) join_s_item<kJoinTile>(work, nt, n, tile, verdict, L);
    } else {  // blocks past the tiles take the hot tiles' overflow items in turn
        const uint32_t nextra = work.item_off[1];
        const uint32_t stride = gridDim.x - tb;
        for (uint32_t xi = blockIdx.x - tb; xi < nextra; xi += stride) {
            __syncthreads();  // the previous item's LDS reads are done
            join_s_item<kJoinItem>(work, nt, n, xi, verdict, L);
        }
    }
    HSC_STAMP(work, 1, 3);
}

hipError_t launch_join_t(const ProbeWork &work, const NarrowTiles &nt, uint32_t n,
                         uint32_t ntiles, uint32_t max_items, uint8_t *verdict, hipStream_t s,
                         uint32_t extra_blocks)
{
    if (max_items == 0 || n == 0 || ntiles == 0) return hipSuccess;
    // one block per tile + up to extra_blocks blocks looping over the
    // overflow items (measured: one block per tile beats persistent blocks
    // that prefetch their next tile -- 27.8 vs 32 us on config 2)
    const uint32_t blocks = join_tile_blocks(ntiles) + std::min<uint32_t>(max_items - ntiles, extra_blocks);
    k_join_t<false><<<blocks, kJoinThreads, 0, s>>>(work, nt, n, ntiles, verdict, nullptr);
    return hipGetLastError();
}

// ---- join: a wave per tile ----
// What the locate's slot filter leaves of most tiles is a few dozen records,
// of which a 512-thread block is mostly barrier.  Here a block serves 8
// consecutive tiles, one per wave.  Prologue, as k_plan_s<true>: the 64-byte
// pieces of the 8 tiles' entries of every chunk row (coalesced) transposed
// into LDS, the block's share of the flag move, and each wave's list -- a quad
// of keys and one of ranks per lane -- into an LDS area of the wave's own; one
// barrier.  Then every wave on its own: scan of its column (8 entries a
// lane), counts[tile], the hot rule, and for a tile of at most kWaveCap kept
// records (two per lane) the chunk search, the record gather, the list vote
// by ballot and the 8-level walk.  The scan leaves {run start << 16 |
// exclusive offset} in the column's LDS words: 16 bits of offset, read only
// where the total is <= kWaveCap.
// A tile of more records, or one whose vote fails, is left alone: its wave
// sets a bit of a block-shared mask, and behind a second barrier the whole
// block runs join_s_item<kJoinCol> for each such tile in turn (its flag move
// off), in LDS that aliases the wave phase's.  A block that falls back for
// kWideBlock tiles or more stores the batch's number into work.wide (the rule
// in hip_serial.h: the next kHotBatches batches take k_join_t<true>).
// LDS: max(wave phase 41,792 B, block phase 40,224 B) + 4: three blocks a CU.
constexpr int kJoinWTiles = kJoinThreads / 64;
constexpr uint32_t kJoinWRow = kMaxChunks + 4;  // a column's words in LDS
constexpr uint32_t kJoinWList = 2 * kRecent + kRecent / 16 + 4;  // a wave's list: keys, ranks, maxima
static_assert(kWaveCap == 2 * 64, "two record slots per lane");
static_assert(kMaxChunks == 8 * 64, "a wave scans a column, 8 entries per lane");
static_assert(kJoinWTiles == 8, "64-byte row pieces, a bit per tile");

__host__ __device__ inline uint32_t join_wave_blocks(uint32_t ntiles)
{
    return 8 * (((ntiles + kJoinWTiles - 1) / kJoinWTiles + 7) / 8);
}

__global__ __launch_bounds__(kJoinThreads) void k_join_w(ProbeWork work, NarrowTiles nt, uint32_t n,
                                                         uint32_t ntiles, uint8_t *verdict,
                                                         uint8_t *flags)
{
    constexpr uint32_t T = 1u << kTLog2;
    constexpr int TB = kJoinWTiles;
    constexpr uint32_t SR = kJoinWRow;
    constexpr uint32_t kWaveWords = TB * SR + TB * kJoinWList + TB * SR / 2;
    constexpr uint32_t kBlockWords = 2 * T + T / 16 + T / 128 + 2 * kRecent + kRecent / 16 + 4 +
                                     2 * kMaxChunks + 4 + 2 * (kJoinThreads / 64);
    __shared__ __attribute__((aligned(16))) uint32_t lds[kWaveWords > kBlockWords ? kWaveWords : kBlockWords];
    __shared__ uint32_t fell;  // bit w: tile t0 + w is left to the block
    // the wave phase
    uint32_t *const sh = lds;                                        // [TB][SR] kept: run start << 16 | count
    uint32_t *const lists = lds + TB * SR;                           // [TB][kJoinWList]
    uint16_t *const shl = (uint16_t *)(lds + TB * SR + TB * kJoinWList);  // [TB][SR] located
    const uint32_t lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    HSC_STAMP(work, 1, 0);
    // neighbouring groups on one XCD, as the tile join's tiles
    const uint32_t t0 = TB * xcd_chunk(blockIdx.x, gridDim.x / 8), t = t0 + w;
    const uint32_t G = work.G, rs = (ntiles + 3) & ~3u;
    const uint32_t fstride = gridDim.x * kJoinThreads, fi = blockIdx.x * kJoinThreads + threadIdx.x;
    // loads first: the first stride's flag, the row pieces (16 bytes: the
    // entries of two tiles), the list
    const uint8_t f0 = fi < work.n_txn ? flags[fi] : 0;
    constexpr int kPieces = kMaxChunks * (TB / 2) / kJoinThreads;  // 4
    u32x4 pc[kPieces];
#pragma unroll
    for (int k = 0; k < kPieces; ++k) {
        const uint32_t i = threadIdx.x + k * kJoinThreads, g = i / (TB / 2), c = t0 + 2 * (i % (TB / 2));
        pc[k] = g < G && c < rs ? *(const u32x4 *)(work.cmx + (size_t)g * rs + c) : u32x4{0, 0, 0, 0};
    }
    uint32_t *const lkeys = lists + w * kJoinWList, *const lrank = lkeys + kRecent;
    uint32_t *const lb16 = lrank + kRecent, *const lb128 = lb16 + kRecent / 16;
    u32x4 lk = {0, 0, 0, 0}, lr = {0, 0, 0, 0};
    uint32_t theta = 0;
    if (t < ntiles) {
        const size_t q = (size_t)t * kRecent + 4 * lane;
        lk = *(const u32x4 *)(nt.rkey32 + q);
        lr = *(const u32x4 *)(nt.rrank32 + q);
        theta = sload(nt.rtheta + t);
    }
    move_flag(work, flags, verdict, fi, f0);
    move_flags_rest(work, flags, verdict, fi, fstride);
    if (t0 >= ntiles) return;  // (block-uniform) a block past the tiles: its flags only
#pragma unroll
    for (int k = 0; k < kPieces; ++k) {
        const uint32_t i = threadIdx.x + k * kJoinThreads, g = i / (TB / 2), c = 2 * (i % (TB / 2));
        if (g < G) {
            sh[c * SR + g] = pc[k].x, sh[(c + 1) * SR + g] = pc[k].z;
            shl[c * SR + g] = (uint16_t)pc[k].y, shl[(c + 1) * SR + g] = (uint16_t)pc[k].w;
        }
    }
    ((u32x4 *)lkeys)[lane] = lk;
    ((u32x4 *)lrank)[lane] = lr;
    {  // the ranks' 16-row maxima (4 lanes) and 128-row maxima (32 lanes)
        uint32_t m = max(max(lr.x, lr.y), max(lr.z, lr.w));
        m = max(m, (uint32_t)__shfl_xor((int)m, 1, 64));
        m = max(m, (uint32_t)__shfl_xor((int)m, 2, 64));
        if ((lane & 3) == 0) lb16[lane >> 2] = m;
#pragma unroll
        for (int d = 4; d < 32; d <<= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
        if ((lane & 31) == 0) lb128[lane >> 5] = m;
    }
    if (threadIdx.x == 0) fell = 0;
    __syncthreads();
    HSC_STAMP(work, 1, 1);
    if (t < ntiles) {
        uint32_t *const col = sh + w * SR;
        const uint16_t *const lcol = shl + w * SR;
        const uint32_t e = 8 * lane;
        uint32_t v[8], c[8], located = 0, sum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t x = e + k < G ? col[e + k] : 0;
            v[k] = x & 0xFFFFu;
            c[k] = x >> 16;
            located += e + k < G ? lcol[e + k] : 0;
            sum += v[k];
        }
        uint32_t x = sum;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) located += __shfl_xor(located, o, 64);
        const uint32_t total = __builtin_amdgcn_readfirstlane(__shfl(x, 63, 64));
        if (lane == 0) work.counts[t] = total;  // (read back by the timing statistics)
        if (lane == 0 && located > kTileCap) mark_hot(work);
        bool fall = total > kWaveCap;  // wave-uniform
        if (!fall && total) {
            uint32_t run = x - sum;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (e + k < G) col[e + k] = c[k] << 16 | run;
                run += v[k];
            }
            // (the wave's own LDS words: written above, searched below by other lanes)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const size_t area = 2 * (size_t)work.chunk;
            u32x4 rec[2];
            bool old = false;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint32_t j = 64 * k + lane;
                rec[k] = u32x4{0, 0, 0, 0};
                if (64u * k >= total) continue;
                uint32_t g = 0;  // offset 0 <= j
#pragma unroll
                for (int b = 8; b >= 0; --b) {
                    const uint32_t cg = g + (1u << b);
                    if (cg < G && (col[cg < G ? cg : 0] & 0xFFFFu) <= j) g = cg;
                }
                if (j < total) {
                    const uint32_t eg = col[g];
                    rec[k] = *(const u32x4 *)(nt.recs + g * area + (eg >> 16) + (j - (eg & 0xFFFFu)));
                }
                // a live record whose snapshot is older than a row left out of the list?
                old |= j < total && rec[k].x <= rec[k].y && rec[k].z < theta;
            }
            fall = __ballot(old) != 0;
            HSC_STAMP(work, 1, 2);
            if (!fall) {
                constexpr uint32_t N = kRecent;
                const uint32_t nrow = min(kRecent, min(T, n - (t << kTLog2)));
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    if (64u * k >= total) continue;
                    const uint32_t lo = rec[k].x, hi = rec[k].y;
                    uint32_t ja = 1, jb = 1;
#pragma unroll
                    for (int d = 0; d < kRecentLog2; ++d) {
                        const uint32_t ka = lkeys[ja], kb = lkeys[jb];
                        ja = 2 * ja + (ka < lo);
                        jb = 2 * jb + (kb <= hi);
                    }
                    const uint32_t kl = lkeys[0];
                    const uint32_t pa = min(ja - N + (kl < lo), nrow);
                    const uint32_t pb = min(jb - N + (kl <= hi), nrow);
                    // A range of at most kShort list rows is read by its own
                    // lane, all of them in one LDS round trip; the wave resolves
                    // only the longer ones, four a pass (stamps on config 2:
                    // a tile's ~50 records nearly all reach the passes
                    // otherwise -- the list's rows are the newest, so their
                    // 16-row maxima pass the two-read filter -- and the walk
                    // phase takes 8.3k cycles of the wave's 19k)
                    constexpr uint32_t kShort = 4;
                    const bool live = 64 * k + lane < total && pa < pb;
                    const bool brief = live && pb - pa <= kShort;
                    bool hit = false;
#pragma unroll
                    for (uint32_t i = 0; i < kShort; ++i) {
                        const bool in = brief && pa + i < pb;
                        hit |= in & (lrank[in ? pa + i : 0] > rec[k].z);
                    }
                    hit |= wave_any_after32(lrank, lb16, lb128, pa, pb, rec[k].z, live && !brief);
                    if (hit) {
                        verdict[rec[k].w] = 1;
                        if (work.bitmap)
                            atomicOr((unsigned long long *)&work.bitmap[rec[k].w >> 6], 1ull << (rec[k].w & 63));
                    }
                }
            }
        }
        if (fall && lane == 0) atomicOr(&fell, 1u << w);
    }
    HSC_STAMP(work, 1, 3);  // (wave 0: its tile's walks are done)
    __syncthreads();
    uint32_t todo = __builtin_amdgcn_readfirstlane(fell);
    if (!todo) return;
    if (threadIdx.x == 0) {
        const uint32_t nfell = __popc(todo);
        if (work.wave_fallbacks) atomicAdd(work.wave_fallbacks, nfell);
        if (nfell >= kWideBlock && work.wide)
            __hip_atomic_store(work.wide, work.batch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // the block phase, over the wave phase's LDS
    uint32_t *o = lds;
    auto take = [&o](uint32_t words) {
        uint32_t *p = o;
        o += words;
        return p;
    };
    JoinLds L;
    L.keys = take(T), L.rank = take(T), L.b16 = take(T / 16), L.b128 = take(T / 128);
    L.lkeys = take(kRecent), L.lrank = take(kRecent), L.lb16 = take(kRecent / 16), L.lb128 = take(4);
    L.Es = take(kMaxChunks), L.Cs = take(kMaxChunks), L.vote = take(4);
    uint32_t *const wtot = take(2 * (kJoinThreads / 64));
    for (bool first = true; todo; todo &= todo - 1, first = false) {
        if (!first) __syncthreads();  // the previous tile's LDS reads are done
        join_s_item<kJoinCol, false>(work, nt, n, t0 + (__ffs(todo) - 1), verdict, L, rs, flags, wtot);
    }
}

hipError_t launch_join_wave(const ProbeWork &work, const NarrowTiles &nt, uint32_t n,
                            uint32_t ntiles, uint8_t *flags, hipStream_t s)
{
    if (n == 0 || ntiles == 0 || !work.vout || !work.cmx || work.G > (uint32_t)kMaxChunks) return hipErrorInvalidValue;
    k_join_w<<<join_wave_blocks(ntiles), kJoinThreads, 0, s>>>(work, nt, n, ntiles, work.vout, flags);
    return hipGetLastError();
}

hipError_t launch_join_col(const ProbeWork &work, const NarrowTiles &nt, uint32_t n,
                           uint32_t ntiles, uint8_t *flags, hipStream_t s)
{
    if (n == 0 || ntiles == 0 || !work.vout || (!work.cmx && !work.cm) || work.G > (uint32_t)kMaxChunks) return hipErrorInvalidValue;
    k_join_t<true><<<join_tile_blocks(ntiles), kJoinThreads, 0, s>>>(work, nt, n, ntiles, work.vout, flags);
    return hipGetLastError();
}

// Verdict bytes of the batch from the conflict flags the probe kernels set
// (an internal array, so nothing has to clear the caller's buffer first):
// verdict[t] = flag, bitmap bit t = flag (one ballot per 64 transactions), and
// set flags are cleared for the next batch.
__global__ void k_pack_flags(uint8_t *flags, uint32_t n, uint8_t *verdict, uint64_t *bitmap)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool v = t < n && flags[t] != 0;
    if (t < n) verdict[t] = v;
    if (v) flags[t] = 0;
    const uint64_t m = __ballot(v);
    if (bitmap && (threadIdx.x & 63) == 0 && t < n) bitmap[t >> 6] = m;
}

hipError_t launch_pack_flags(uint8_t *flags, uint32_t n_txn, uint8_t *verdict, uint64_t *bitmap,
                             hipStream_t s)
{
    if (n_txn == 0) return hipSuccess;
    k_pack_flags<<<(n_txn + 255) / 256, 256, 0, s>>>(flags, n_txn, verdict, bitmap);
    return hipGetLastError();
}

// load this file's code object now (HIP loads it lazily at the first launch
// of one of its kernels: ~1 ms, which would land inside the first build or
// probe -- hsc_ctx_create calls every warm_* once)
hipError_t warm_narrow()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_end_rows);
}

}  // namespace hsc
