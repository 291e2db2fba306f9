// hsc_linear_wide.hip -- the wide tier of the linearizability search (DESIGN.md
// §5j): hsc_linear.hip's step -- seed, sweeps, rebuild, the all-hold-i fast
// path, the same event order and counts of sets -- for the keys whose search
// leaves LDS, with the two hash sets in device memory.  One workgroup per key,
// one launch per round of keys, nothing shared across workgroups.
//
// A configuration is one uint64_t, so an insert is still one 64-bit
// compare-and-swap: bit 63 the work table's "unexpanded" tag, bits 62-48 the
// register's state id (0 = nil, at most kLinWideStates values), bits 47-0 the
// pending slots already linearized (kLinWideSlots).  A tagged entry lacks the
// returning op's bit, so no entry equals the empty word ~0.
//
// Tables.  A key owns 4 * max_configs words of the arena: two sets of
// 2 * max_configs.  They are used at a power-of-two size from kLinMinTable up
// with k_linear's protocol: an insert that takes the entry count past half the
// size in use, or finds no free slot in one cycle of the table, raises the
// overflow flag, which a sweep reads before every expansion; the step is then
// redone one size up from the untouched set, and past max_configs entries at
// the largest size the key is UNKNOWN / configs.  The flag is exact: raised iff
// the closure has more entries than the limit.  LDS holds the pending table,
// the staged events and the control words.
//
// Budget.  After every completed step, a key whose expansions so far exceed
// max_expanded is UNKNOWN / budget.  The default, 2^25 (kLinWideDefaultBudget),
// is the largest power of two one key does in under ten seconds (5.7 s) at the
// rate measured on 2^20 configurations in one step, 5.9 M expansions/s
// (2^26 would be 11.4 s).
//
// 1024 threads: the bench's two shapes took 1.7x and 1.8x as long at 512.
//
// Memory rules.
//  * Every read of a table word is a relaxed agent-scope atomic load
//    (tab_load): in a sweep the word may be written by another wave's
//    compare-and-swap in the same phase, and the atomics execute in L2, so a
//    plain load could be served a stale line from the CU's L1.  The other
//    reads (seed, rebuild, copy, the BAD key's states) are of words written
//    in an earlier phase and take the same path, so no table read depends on
//    what L1 holds.
//  * Table words are written by the compare-and-swap of an insert, the atomic
//    AND that clears a tag (by the slot's owner only), and the plain stores of
//    a clear, which no other thread reads or writes in that phase.
//  * Phases are separated by __syncthreads().  The tables are cleared in the
//    kernel; the host does not initialise the arena.
//  * No spin-waits: no thread waits for another outside a barrier.
//  * Every loop has a bound, so a launch always ends: the events (nev); the
//    redo of a step (the table sizes, at most 16); the sweeps of a step (an
//    entry is expanded once, and each sweep but the last expands at least
//    one: at most the table's entries); a probe (one cycle of the table); the
//    candidates of an entry (48).  max_expanded bounds the expansions.
//  * Plain HIP and atomics only; the result words are plain stores of thread 0.
#include "hsc_linear_dev.h"

namespace hsc {

namespace {

constexpr uint64_t kWideEmpty = ~0ull;
constexpr uint64_t kWideTag = 1ull << 63;
constexpr uint64_t kWideMask = (1ull << kLinWideSlots) - 1;
constexpr int kWideStateShift = 48;
constexpr uint32_t kWideBatch = 4;  // slots a thread reads ahead in a sweep
// control words in LDS
enum { kCnt = 0, kOvf, kAlive, kExp, kDone, kCtl };

__device__ __forceinline__ uint64_t tab_load(const uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t wide_state(uint64_t c) { return (uint32_t)(c >> kWideStateShift) & 0x7FFFu; }

__device__ __forceinline__ uint64_t wide_word(uint32_t state, uint64_t mask)
{
    return (uint64_t)state << kWideStateShift | mask;
}

// key into t[size] unless it is there (the tag does not tell entries apart);
// counted in ctl[kCnt].  More than `limit` entries, or no free slot: ctl[kOvf]
// (k_linear's lin_insert, on device memory).
__device__ void wide_insert(uint64_t *t, uint32_t size, uint64_t key, uint32_t limit, uint32_t *ctl)
{
    volatile uint32_t *vc = ctl;
    uint32_t h = lin_hash(key & ~kWideTag) & (size - 1);
    for (uint32_t n = 0; n < size; ++n) {
        const uint64_t old = atomicCAS((unsigned long long *)&t[h], kWideEmpty, key);
        if (old == kWideEmpty) {
            if (atomicAdd(&ctl[kCnt], 1u) + 1 > limit) vc[kOvf] = 1;
            return;
        }
        if (((old ^ key) & ~kWideTag) == 0) return;
        h = (h + 1) & (size - 1);
    }
    vc[kOvf] = 1;
}

// the least table size that holds n entries at load <= 1/2
__device__ __forceinline__ uint32_t wide_fit(uint32_t n, uint32_t largest)
{
    uint32_t s = kLinMinTable;
    while (s < 2 * n && s < largest) s <<= 1;
    return s;
}

__global__ __launch_bounds__(kLinWideThreads) void k_linear_wide(const LinEvent *__restrict__ prog,
                                                                 const LinKey *__restrict__ keys,
                                                                 LinResult *__restrict__ res,
                                                                 uint8_t *__restrict__ seen, uint64_t *tables,
                                                                 uint32_t max_configs, uint64_t max_expanded)
{
    __shared__ uint32_t pf[kLinWideSlots], pa[kLinWideSlots], pb[kLinWideSlots];
    __shared__ uint32_t ctl[kCtl];
    __shared__ unsigned long long mask_and;  // the AND of the rebuilt set's masks
    __shared__ LinEvent evbuf[kLinEvBuf];    // the next events of the program, staged kLinEvBuf at a time
    volatile uint32_t *vc = ctl;
    constexpr uint32_t T = kLinWideThreads;
    const uint32_t tid = threadIdx.x;
    const LinKey k = keys[blockIdx.x];
    const uint32_t largest = 2 * max_configs;  // words of one table
    uint64_t *const tab0 = tables + (size_t)blockIdx.x * 2 * largest, *const tab1 = tab0 + largest;

    int cur = 0;                       // the table that holds the set
    uint32_t csize = kLinMinTable;     // its size in use
    uint32_t ccount = 1;               // its entries
    uint64_t allmask = 0;              // the AND of their masks
    uint64_t pend = 0;                 // slots with a pending op
    uint32_t peak = 1;
    uint64_t expanded = 0;
    uint32_t verdict = HSC_LIN_OK, cause = 0, fail_ev = 0xFFFFFFFFu;

    for (uint32_t s = tid; s < csize; s += T) tab0[s] = kWideEmpty;
    __syncthreads();
    if (tid == 0) tab0[lin_hash(wide_word(k.init, 0)) & (csize - 1)] = wide_word(k.init, 0);
    __syncthreads();

    for (uint32_t e = 0; e < k.nev; ++e) {
        if (e % kLinEvBuf == 0) {
            __syncthreads();  // (every thread has read the last event of the chunk before)
            for (uint32_t j = tid; j < min(kLinEvBuf, k.nev - e); j += T) evbuf[j] = prog[k.ev_off + e + j];
            __syncthreads();
        }
        const LinEvent ev = evbuf[e % kLinEvBuf];
        const uint32_t i = ev.w >> 1 & 63u;
        const uint64_t bit = 1ull << i;
        if (!(ev.w & 1u)) {  // a call (the step that ended before it ended with a barrier)
            if (tid == 0) pf[i] = ev.w >> 8 & 3u, pa[i] = ev.a, pb[i] = ev.b;
            pend |= bit;
            continue;
        }
        uint64_t *const C = cur ? tab1 : tab0, *const W = cur ? tab0 : tab1;
        if (allmask & bit) {  // every configuration holds i
            const uint32_t wsize = wide_fit(ccount, largest);
            for (uint32_t s = tid; s < wsize; s += T) W[s] = kWideEmpty;
            if (tid == 0) ctl[kCnt] = 0, ctl[kOvf] = 0;
            __syncthreads();
            for (uint32_t s = tid; s < csize; s += T) {
                const uint64_t c = tab_load(&C[s]);
                if (c != kWideEmpty) wide_insert(W, wsize, c & ~bit, wsize / 2, ctl);
            }
            __syncthreads();
            cur ^= 1;
            csize = wsize;
            allmask &= ~bit;
            pend &= ~bit;
            continue;
        }
        __syncthreads();  // the pending table holds every call before this return
        const uint32_t fi = pf[i], ai = pa[i], bi = pb[i];
        uint32_t wsize = wide_fit(2 * ccount, largest), wcount = 0, wdone = 0;
        bool over = false, alive = false;
        for (;;) {  // the step, again one size up while the work table overflows
            const uint32_t limit = wsize / 2;
            for (uint32_t s = tid; s < wsize; s += T) W[s] = kWideEmpty;
            if (tid == 0) ctl[kCnt] = 0, ctl[kOvf] = 0, ctl[kAlive] = 0, ctl[kExp] = 0, ctl[kDone] = 0;
            __syncthreads();
            // seed
            uint32_t ndone = 0;
            for (uint32_t s = tid; s < csize; s += T) {
                const uint64_t c = tab_load(&C[s]);
                if (c == kWideEmpty) continue;
                const bool has = (c & bit) != 0;
                ndone += has;
                wide_insert(W, wsize, has ? c : c | kWideTag, limit, ctl);
            }
            if (ndone) atomicAdd(&ctl[kDone], ndone), vc[kAlive] = 1;
            __syncthreads();
            // sweeps
            for (;;) {
                uint32_t nexp = 0;
                bool stop = false;
                for (uint32_t s0 = tid; s0 < wsize && !stop; s0 += kWideBatch * T) {
                    uint64_t t[kWideBatch];
#pragma unroll
                    for (uint32_t u = 0; u < kWideBatch; ++u) {
                        const uint32_t s = s0 + u * T;
                        t[u] = s < wsize ? tab_load(&W[s]) : kWideEmpty;
                    }
#pragma unroll
                    for (uint32_t u = 0; u < kWideBatch; ++u) {
                        if (stop || t[u] == kWideEmpty || !(t[u] & kWideTag)) continue;
                        if (vc[kOvf]) {
                            stop = true;
                            continue;
                        }
                        atomicAnd((unsigned long long *)&W[s0 + u * T], ~kWideTag);
                        ++nexp;
                        const uint32_t st = wide_state(t[u]);
                        const uint64_t mask = t[u] & kWideMask;
                        uint32_t ns;
                        if (lin_apply(fi, ai, bi, st, &ns)) vc[kAlive] = 1;
                        for (uint64_t cand = pend & ~mask & ~bit; cand; cand &= cand - 1) {
                            const uint32_t j = (uint32_t)__builtin_ctzll(cand);
                            if (lin_apply(pf[j], pa[j], pb[j], st, &ns))
                                wide_insert(W, wsize, wide_word(ns, mask | 1ull << j) | kWideTag, limit, ctl);
                        }
                    }
                }
                if (nexp) atomicAdd(&ctl[kExp], nexp);
                __syncthreads();
                wcount = ctl[kCnt];
                wdone = ctl[kDone];
                const uint32_t wexp = ctl[kExp];
                over = ctl[kOvf] != 0;
                alive = ctl[kAlive] != 0;
                __syncthreads();
                if (over || wexp == wcount - wdone) break;
            }
            if (!over || wsize == largest) break;
            wsize <<= 1;
        }
        if (over) {
            verdict = HSC_LIN_UNKNOWN, cause = HSC_LIN_CAUSE_CONFIGS;
            break;
        }
        peak = max(peak, wcount);
        expanded += wcount - wdone;
        if (!alive) {
            verdict = HSC_LIN_BAD, fail_ev = e;
            for (uint32_t s = tid; s < csize; s += T) {
                const uint64_t c = tab_load(&C[s]);
                if (c != kWideEmpty) seen[k.seen_off + wide_state(c)] = 1;
            }
            break;
        }
        // rebuild the set in place of the old one
        for (uint32_t s = tid; s < wsize; s += T) C[s] = kWideEmpty;
        if (tid == 0) ctl[kCnt] = 0, ctl[kOvf] = 0, mask_and = kWideMask;
        __syncthreads();
        uint64_t mand = kWideMask;
        for (uint32_t s = tid; s < wsize; s += T) {
            const uint64_t t = tab_load(&W[s]);
            if (t == kWideEmpty) continue;
            const uint32_t st = wide_state(t);
            const uint64_t mask = t & kWideMask;
            uint32_t ns = st;
            if (!(mask & bit) && !lin_apply(fi, ai, bi, st, &ns)) continue;
            const uint64_t nm = mask & ~bit;
            mand &= nm;
            wide_insert(C, wsize, wide_word(ns, nm), wsize / 2, ctl);
        }
        if (mand != kWideMask) atomicAnd(&mask_and, (unsigned long long)mand);
        __syncthreads();
        ccount = vc[kCnt];
        allmask = *(volatile unsigned long long *)&mask_and;
        csize = wsize;
        pend &= ~bit;
        __syncthreads();
        if (expanded > max_expanded) {  // (the same sum in every thread)
            verdict = HSC_LIN_UNKNOWN, cause = HSC_LIN_CAUSE_BUDGET;
            break;
        }
    }
    if (tid == 0) {
        LinResult r;
        r.verdict = verdict, r.cause = cause, r.fail_ev = fail_ev;
        r.peak = peak, r.final_n = ccount;
        r.expanded_lo = (uint32_t)expanded, r.expanded_hi = (uint32_t)(expanded >> 32);
        r.pad = 0;
        res[blockIdx.x] = r;
    }
}

}  // namespace

hipError_t linear_search_wide(const LinEvent *prog, const LinKey *keys, uint32_t nkeys, LinResult *res, uint8_t *seen,
                              uint64_t *tables, const LinWideLimits &lim, hipStream_t s)
{
    if (!nkeys) return hipSuccess;
    hipLaunchKernelGGL(k_linear_wide, dim3(nkeys), dim3(kLinWideThreads), 0, s, prog, keys, res, seen, tables,
                       lim.max_configs, lim.max_expanded);
    return hipGetLastError();
}

// load this file's code object now (see warm_graph)
hipError_t warm_linear_wide()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_linear_wide);
}

}  // namespace hsc
