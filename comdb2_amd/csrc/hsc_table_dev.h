// hsc_table_dev.h -- device helpers shared by the value-history entries
// (hsc_resolve.hip, hsc_lists.hip): the per-workgroup counter sums and the
// search of the written (key, value) table through its key directory.
#pragma once
#include "hsc_device.h"

namespace hsc {

constexpr int kRvThreads = 256;
constexpr uint64_t kRvFin = 1ull << 63;  // table payload: the txn's final write of the key

// Sums v[q] over the workgroup (kRvThreads threads) and adds every sum that is
// not zero to dst[q] (every thread of the workgroup calls this).
template <int N>
__device__ __forceinline__ void block_add(uint32_t (&v)[N], unsigned long long *dst, uint32_t (*lds)[N])
{
    const int lane = lane_id(), wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        uint32_t x = v[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) lds[wid][q] = x;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kRvThreads / 64; ++w) t += lds[w][threadIdx.x];
        if (t) atomicAdd(dst + threadIdx.x, (unsigned long long)t);
    }
}

// bucket of key k over [kmin, kmin + span]: (k - kmin) >> shift, below 2^D
// (shift = 64: one bucket over a span of 64 bits)
__device__ __forceinline__ int rv_dir_shift(uint64_t span, int D)
{
    const int bits = span ? 64 - __clzll((long long)span) : 0;
    return bits > D ? bits - D : 0;
}
__device__ __forceinline__ uint64_t rv_shr(uint64_t x, int shift) { return shift >= 64 ? 0 : x >> shift; }
__device__ __forceinline__ uint64_t rv_shl(uint64_t x, int shift) { return shift >= 64 ? 0 : x << shift; }

// The row of (k, v) in the table of nw rows sorted by (tk, tv), through the
// directory of 2^D key buckets (every row of a key lies in one bucket; a
// history with one hot key degrades to the plain binary search); nw: no such
// row.
__device__ __forceinline__ size_t rv_find(size_t nw, const uint64_t *tk, const uint64_t *tv, int D,
                                          const uint32_t *dir, uint64_t k, uint64_t v)
{
    size_t lo = 0, hi = 0;
    if (nw) {
        const uint64_t kmin = tk[0], span = tk[nw - 1] - kmin;
        if (k >= kmin && k - kmin <= span) {
            const uint32_t b = (uint32_t)rv_shr(k - kmin, rv_dir_shift(span, D));
            lo = dir[b];
            hi = dir[b + 1];
        }
    }
    const size_t end = hi;
    while (lo < hi) {  // the bucket's first row >= (k, v)
        const size_t mid = lo + ((hi - lo) >> 1);
        const uint64_t mk = tk[mid];
        const bool less = mk < k || (mk == k && tv[mid] < v);
        if (less)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < end && tk[lo] == k && tv[lo] == v ? lo : nw;
}

}  // namespace hsc
