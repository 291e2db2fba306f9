// hsc_linear.hip -- linearizability of a compare-and-set register history
// (DESIGN.md §5j): knossos.linear's just-in-time search over configurations
// (linearizable/jepsen/src/knossos/linear.clj:66-129, 218-271), one workgroup
// per key, the key's whole search in one launch.
//
// A configuration is one uint64_t: the register's state id in the high word
// (ids stay below 2^31; bit 63 is the work table's "unexpanded" tag), the
// pending slots already linearized in the low word.  The workgroup keeps the
// current set and a step's work table as two open-addressing hash sets in LDS
// (kLinTable slots each, used at a power-of-two size from kLinMinTable up, load
// <= 1/2) and the pending ops' table beside them.  A set is scanned, not
// listed: thread t owns the slots t, t + kLinThreads, ...
//
// The events are staged through LDS kLinEvBuf at a time (one coalesced read a
// chunk, not a dependent global read an event).
// A call stores the op in the pending table.  A return of slot i:
//   fast     every configuration holds i (the AND of the set's masks, kept by
//            the rebuild): copy the set into the other table with the bit
//            cleared; the tables change roles
//   seed     the work table := the set; entries without bit i tagged
//   sweep    until every entry is expanded: a tagged entry's owner clears the
//            tag, notes whether i is legal on it, and inserts its legal
//            successors by every pending j != i outside its mask, tagged.  An
//            entry inserted behind the owner's position waits for the next
//            sweep; masks only grow, so this ends
//   rebuild  no entry holds i or can take it: the key fails here, the set stays
//            as it stood.  Else the set := the entries with bit i, cleared, and
//            the i-successors of the others
// A work table that passes load 1/2 ends the step, which starts again one size
// up; past kLinCap entries at the largest size the key is UNKNOWN.
// The counts -- a step's entries, the entries expanded, the set's size -- are
// of sets, so they do not depend on the order of insertion.
//
// Only LDS atomics (the 64-bit compare-and-swap of an insert, the counters);
// the result words are plain stores of thread 0.
#include "hsc_linear_dev.h"

namespace hsc {

namespace {

constexpr uint64_t kLinEmpty = ~0ull;
constexpr uint64_t kLinTag = 1ull << 63;
// control words in LDS
enum { kCnt = 0, kOvf, kAlive, kExp, kDone, kAnd, kCtl };

// key into t[size] unless it is there (the tag does not tell entries apart);
// counted in ctl[kCnt].  More than `limit` entries, or no free slot: ctl[kOvf],
// which a sweep reads before every expansion -- what is inserted past the
// limit until every thread has seen it may fill the table, never more: the
// probe gives up after one cycle.
__device__ void lin_insert(uint64_t *t, uint32_t size, uint64_t key, uint32_t limit, uint32_t *ctl)
{
    volatile uint32_t *vc = ctl;
    uint32_t h = lin_hash(key & ~kLinTag) & (size - 1);
    for (uint32_t n = 0; n < size; ++n) {
        const uint64_t old = atomicCAS((unsigned long long *)&t[h], kLinEmpty, key);
        if (old == kLinEmpty) {
            if (atomicAdd(&ctl[kCnt], 1u) + 1 > limit) vc[kOvf] = 1;
            return;
        }
        if (((old ^ key) & ~kLinTag) == 0) return;
        h = (h + 1) & (size - 1);
    }
    vc[kOvf] = 1;
}

// the least table size that holds n entries at load <= 1/2
__device__ __forceinline__ uint32_t lin_fit(uint32_t n)
{
    uint32_t s = kLinMinTable;
    while (s < 2 * n && s < kLinTable) s <<= 1;
    return s;
}

__global__ __launch_bounds__(kLinThreads) void k_linear(const LinEvent *__restrict__ prog,
                                                        const LinKey *__restrict__ keys,
                                                        LinResult *__restrict__ res, uint8_t *__restrict__ seen)
{
    __shared__ uint64_t tab[2][kLinTable];
    __shared__ uint32_t pf[kLinSlots], pa[kLinSlots], pb[kLinSlots];
    __shared__ uint32_t ctl[kCtl];
    __shared__ LinEvent evbuf[kLinEvBuf];  // the next events of the program, staged kLinEvBuf at a time
    volatile uint32_t *vc = ctl;
    const uint32_t tid = threadIdx.x;
    const LinKey k = keys[blockIdx.x];

    int cur = 0;                       // the table that holds the set
    uint32_t csize = kLinMinTable;     // its size in use
    uint32_t ccount = 1;               // its entries
    uint32_t allmask = 0;              // the AND of their masks
    uint32_t pend = 0;                 // slots with a pending op
    uint32_t peak = 1;
    uint64_t expanded = 0;
    uint32_t verdict = HSC_LIN_OK, cause = 0, fail_ev = 0xFFFFFFFFu;

    for (uint32_t s = tid; s < csize; s += kLinThreads) tab[0][s] = kLinEmpty;
    __syncthreads();
    if (tid == 0) tab[0][lin_hash((uint64_t)k.init << 32) & (csize - 1)] = (uint64_t)k.init << 32;
    __syncthreads();

    for (uint32_t e = 0; e < k.nev; ++e) {
        if (e % kLinEvBuf == 0) {
            __syncthreads();  // (every thread has read the last event of the chunk before)
            for (uint32_t j = tid; j < min(kLinEvBuf, k.nev - e); j += kLinThreads) evbuf[j] = prog[k.ev_off + e + j];
            __syncthreads();
        }
        const LinEvent ev = evbuf[e % kLinEvBuf];
        const uint32_t i = ev.w >> 1 & 31u, bit = 1u << i;
        if (!(ev.w & 1u)) {  // a call (the step that ended before it ended with a barrier)
            if (tid == 0) pf[i] = ev.w >> 8 & 3u, pa[i] = ev.a, pb[i] = ev.b;
            pend |= bit;
            continue;
        }
        uint64_t *const C = tab[cur], *const W = tab[cur ^ 1];
        if (allmask & bit) {  // every configuration holds i
            const uint32_t wsize = lin_fit(ccount);
            for (uint32_t s = tid; s < wsize; s += kLinThreads) W[s] = kLinEmpty;
            if (tid == 0) ctl[kCnt] = 0, ctl[kOvf] = 0;
            __syncthreads();
            for (uint32_t s = tid; s < csize; s += kLinThreads) {
                const uint64_t c = C[s];
                if (c != kLinEmpty) lin_insert(W, wsize, c & ~(uint64_t)bit, wsize / 2, ctl);
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
        uint32_t wsize = lin_fit(2 * ccount), wcount = 0, wdone = 0;
        bool over = false, alive = false;
        for (;;) {  // the step, again one size up while the work table overflows
            const uint32_t limit = wsize / 2;
            for (uint32_t s = tid; s < wsize; s += kLinThreads) W[s] = kLinEmpty;
            if (tid == 0) ctl[kCnt] = 0, ctl[kOvf] = 0, ctl[kAlive] = 0, ctl[kExp] = 0, ctl[kDone] = 0;
            __syncthreads();
            // seed
            uint32_t ndone = 0;
            for (uint32_t s = tid; s < csize; s += kLinThreads) {
                const uint64_t c = C[s];
                if (c == kLinEmpty) continue;
                const bool has = ((uint32_t)c & bit) != 0;
                ndone += has;
                lin_insert(W, wsize, has ? c : c | kLinTag, limit, ctl);
            }
            if (ndone) atomicAdd(&ctl[kDone], ndone), vc[kAlive] = 1;
            __syncthreads();
            // sweeps
            for (;;) {
                uint32_t nexp = 0;
                for (uint32_t s = tid; s < wsize; s += kLinThreads) {
                    const uint64_t t = ((volatile uint64_t *)W)[s];
                    if (t == kLinEmpty || !(t & kLinTag)) continue;
                    if (vc[kOvf]) break;
                    atomicAnd((unsigned long long *)&W[s], ~kLinTag);
                    ++nexp;
                    const uint32_t st = (uint32_t)(t >> 32) & 0x7FFFFFFFu, mask = (uint32_t)t;
                    uint32_t ns;
                    if (lin_apply(fi, ai, bi, st, &ns)) vc[kAlive] = 1;
                    for (uint32_t cand = pend & ~mask & ~bit; cand; cand &= cand - 1) {
                        const uint32_t j = __builtin_ctz(cand);
                        if (lin_apply(pf[j], pa[j], pb[j], st, &ns))
                            lin_insert(W, wsize, (uint64_t)ns << 32 | mask | 1u << j | kLinTag, limit, ctl);
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
            if (!over || wsize == kLinTable) break;
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
            for (uint32_t s = tid; s < csize; s += kLinThreads) {
                const uint64_t c = C[s];
                if (c != kLinEmpty) seen[k.seen_off + (uint32_t)(c >> 32)] = 1;
            }
            break;
        }
        // rebuild the set in place of the old one
        for (uint32_t s = tid; s < wsize; s += kLinThreads) C[s] = kLinEmpty;
        if (tid == 0) ctl[kCnt] = 0, ctl[kAnd] = 0xFFFFFFFFu;
        __syncthreads();
        uint32_t mand = 0xFFFFFFFFu;
        for (uint32_t s = tid; s < wsize; s += kLinThreads) {
            const uint64_t t = W[s];
            if (t == kLinEmpty) continue;
            const uint32_t st = (uint32_t)(t >> 32) & 0x7FFFFFFFu, mask = (uint32_t)t;
            uint32_t ns = st;
            if (!(mask & bit) && !lin_apply(fi, ai, bi, st, &ns)) continue;
            const uint32_t nm = mask & ~bit;
            mand &= nm;
            lin_insert(C, wsize, (uint64_t)ns << 32 | nm, wsize / 2, ctl);
        }
        if (mand != 0xFFFFFFFFu) atomicAnd(&ctl[kAnd], mand);
        __syncthreads();
        ccount = vc[kCnt];
        allmask = vc[kAnd];
        csize = wsize;
        pend &= ~bit;
        __syncthreads();
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

hipError_t linear_search(const LinEvent *prog, const LinKey *keys, uint32_t nkeys, LinResult *res, uint8_t *seen,
                         hipStream_t s)
{
    if (!nkeys) return hipSuccess;
    hipLaunchKernelGGL(k_linear, dim3(nkeys), dim3(kLinThreads), 0, s, prog, keys, res, seen);
    return hipGetLastError();
}

// load this file's code object now (see warm_graph)
hipError_t warm_linear()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_linear);
}

}  // namespace hsc
