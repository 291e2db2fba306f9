// hsc_perf.hip -- the reference's checker/perf: the data sets
// of jepsen/checker/perf.clj's three graphs and its rate breakdown from one
// timed history.  Neither a graph nor a search: two sorts (a third and a
// fourth for the rate cells and, on request, the raw partition) and flag +
// scan passes.
//
// Passes (the discipline of hsc_tally.hip and hsc_intcons.hip: flag +
// scan_exclusive_u32 compaction, so every output is in a defined order; plain
// stores; the only atomics are the counters and the time maximum, one per
// workgroup and value that is not zero):
//   rows      one row (process, 0) with the op's index as payload; the input
//             checks; the invokes counted, the completions flagged
//   pair      sort_rows2 (stable) by process, then one kernel over adjacent
//             sorted rows: an op that is no invoke pairs with the row before it
//             iff that row has the same process and is an invoke -- what
//             util/history->latencies' map from process to its outstanding
//             invoke comes to.  completion_of / invoke_of / latency per op
//   cells     the paired invokes compacted to rows ((f, window), latency ^ sign
//             bit) and sorted; the cell heads flagged and scanned, a cell's
//             length the distance to the next head (no thread loops over a
//             cell); per listed cell and q the element at min(n - 1, floor(n q))
//   rate      the ops that are no invoke compacted to rows keyed (f, type, not
//             client, window) and sorted; the heads of the client cells listed
//             as above; the (f, type) group offsets, which give the counts
//             matrix of all of them, from adjacent keys
//   raw       (on request) the paired invokes keyed f * 4 + the completion's
//             type and sorted (stable: history order inside a group), the
//             group offsets from adjacent keys
#include <algorithm>
#include <cmath>

#include "hsc_internal.h"
#include "hsc_table_dev.h"

namespace hsc {

namespace {

constexpr uint64_t kPfSign = 1ull << 63;
enum { kPfBad, kPfInvokes, kPfPaired, kPfOrphans, kPfN, kPfTmax = kPfN, kPfWords };

inline unsigned pf_blocks(size_t n) { return (unsigned)((n + kRvThreads - 1) / kRvThreads); }

// The window of time t (ns, >= 0) under dt seconds: the reference's two double
// divisions (perf.clj:15-25 after util/nanos->secs), truncated.  false: past
// the accepted windows.
__device__ __forceinline__ bool pf_bucket(int64_t t, double dt, uint32_t *b)
{
    const double w = ((double)t / 1e9) / dt;
    if (!(w < 4294967296.0)) return false;
    *b = (uint32_t)(long long)w;
    return true;
}

// cflag: [n + 1] the ops that are no invoke (0 at n)
__global__ __launch_bounds__(kRvThreads) void k_pf_rows(size_t n, const uint8_t *type, const uint32_t *f,
                                                        const uint32_t *proc, const int64_t *time, uint32_t nf,
                                                        double q_dt, double r_dt, size_t cap, uint64_t *rows,
                                                        uint64_t *pay, uint32_t *cflag, unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][2];
    __shared__ unsigned long long mx[kRvThreads / 64];
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[2] = {0, 0};
    unsigned long long m = 0;
    if (i < n) {
        const uint8_t ty = type[i];
        const int64_t t = time[i];
        uint32_t b;
        v[kPfBad] = ty > HSC_OP_INFO || f[i] >= nf || t < 0 || !pf_bucket(t, q_dt, &b) || !pf_bucket(t, r_dt, &b);
        v[kPfInvokes] = ty == HSC_OP_INVOKE;
        m = t < 0 ? 0 : (unsigned long long)t;
        rows[i] = proc[i];
        rows[cap + i] = 0;
        pay[i] = i;
        cflag[i] = ty != HSC_OP_INVOKE;
    } else if (i == n) {
        cflag[i] = 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
    if (lane_id() == 0) mx[threadIdx.x >> 6] = m;
    block_add<2>(v, ct, lds);  // (its barrier orders mx too)
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < kRvThreads / 64; ++w) t = max(t, mx[w]);
        if (t) atomicMax(ct + kPfTmax, t);
    }
}

// ws / ps: the rows sorted by process (stable) and their op indices.
// pflag: [n + 1] the paired invokes, by op (0 at n)
__global__ __launch_bounds__(kRvThreads) void k_pf_pair(size_t n, const uint64_t *ws, const uint64_t *ps,
                                                        const uint8_t *type, const int64_t *time, int32_t *comp,
                                                        int32_t *inv, int64_t *lat, uint32_t *pflag,
                                                        unsigned long long *ct)
{
    __shared__ uint32_t lds[kRvThreads / 64][2];
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    uint32_t v[2] = {0, 0};  // paired, orphans
    if (q < n) {
        const uint32_t i = (uint32_t)ps[q];
        if (type[i] == HSC_OP_INVOKE) {
            int32_t j = -1;
            if (q + 1 < n && ws[q + 1] == ws[q]) {
                const uint32_t k = (uint32_t)ps[q + 1];
                if (type[k] != HSC_OP_INVOKE) j = (int32_t)k;
            }
            comp[i] = j;
            inv[i] = -1;
            lat[i] = j < 0 ? 0 : (int64_t)((uint64_t)time[j] - (uint64_t)time[i]);
            pflag[i] = j >= 0;
            v[0] = j >= 0;
        } else {
            int32_t j = -1;
            if (q > 0 && ws[q - 1] == ws[q]) {
                const uint32_t k = (uint32_t)ps[q - 1];
                if (type[k] == HSC_OP_INVOKE) j = (int32_t)k;
            }
            comp[i] = -1;
            inv[i] = j;
            lat[i] = 0;
            pflag[i] = 0;
            v[1] = j < 0;
        }
    } else if (q == n) {
        pflag[n] = 0;
    }
    block_add<2>(v, ct + kPfPaired, lds);
}

// pos: pflag scanned.  Row p of paired invoke i: ((f, window of its time), latency ^ sign bit)
__global__ __launch_bounds__(kRvThreads) void k_pf_latrows(size_t n, const uint32_t *pos, const uint32_t *f,
                                                           const int64_t *time, const int64_t *lat, double q_dt,
                                                           size_t cap, uint64_t *rows, uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p) return;
    uint32_t b = 0;
    (void)pf_bucket(time[i], q_dt, &b);  // (k_pf_rows accepted it)
    rows[p] = (uint64_t)f[i] << 32 | b;
    rows[cap + p] = (uint64_t)lat[i] ^ kPfSign;
    pay[p] = i;
}

// pos: pflag scanned.  Row p of paired invoke i: (f * 4 + its completion's type, 0)
__global__ __launch_bounds__(kRvThreads) void k_pf_rawrows(size_t n, const uint32_t *pos, const uint32_t *f,
                                                           const uint8_t *type, const int32_t *comp, size_t cap,
                                                           uint64_t *rows, uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p) return;
    rows[p] = (uint64_t)f[i] * 4 + type[comp[i]];
    rows[cap + p] = 0;
    pay[p] = i;
}

// pos: cflag scanned.  Row p of completion i: (f << 35 | type << 33 | not client << 32 | window, 0)
__global__ __launch_bounds__(kRvThreads) void k_pf_raterows(size_t n, const uint32_t *pos, const uint32_t *f,
                                                            const uint8_t *type, const uint8_t *client,
                                                            const int64_t *time, double r_dt, size_t cap,
                                                            uint64_t *rows, uint64_t *pay)
{
    const size_t i = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = pos[i];
    if (pos[i + 1] == p) return;
    uint32_t b = 0;
    (void)pf_bucket(time[i], r_dt, &b);
    rows[p] = (uint64_t)f[i] << 35 | (uint64_t)type[i] << 33 | (uint64_t)(client[i] == 0) << 32 | b;
    rows[cap + p] = 0;
    pay[p] = i;
}

// h0[q] / h1[q] (q <= m; 0 at m): the sorted position q heads a cell / a cell
// whose key has none of skip's bits (h1 may be h0 when skip is 0)
__global__ __launch_bounds__(kRvThreads) void k_pf_heads(size_t m, const uint64_t *ws, uint64_t skip, uint32_t *h0,
                                                         uint32_t *h1)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > m) return;
    const bool head = q < m && (q == 0 || ws[q] != ws[q - 1]);
    h0[q] = head;
    if (h1 != h0) h1[q] = head && !(ws[q] & skip);
}

// h0 scanned: cpos[k] = the k-th cell's first position (cpos[cells] = m)
__global__ __launch_bounds__(kRvThreads) void k_pf_cpos(size_t m, const uint32_t *h0, uint32_t *cpos)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > m) return;
    const uint32_t k = h0[q];
    if (q == m)
        cpos[k] = (uint32_t)m;
    else if (h0[q + 1] != k)
        cpos[k] = (uint32_t)q;
}

// One thread per (listed cell k, quantile j); nq1 = max(nq, 1)
__global__ __launch_bounds__(kRvThreads) void k_pf_quant(uint32_t ncl, uint32_t nq, uint32_t nq1, const double *qs,
                                                         const uint64_t *ws, size_t cap, const uint32_t *cpos,
                                                         uint32_t *c_f, uint32_t *c_b, uint32_t *c_n, int64_t *c_lat)
{
    const size_t t = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (t >= (size_t)ncl * nq1) return;
    const uint32_t k = (uint32_t)(t / nq1), j = (uint32_t)(t % nq1);
    const uint32_t p = cpos[k], cnt = cpos[k + 1] - p;
    if (j == 0) {
        const uint64_t key = ws[p];
        c_f[k] = (uint32_t)(key >> 32);
        c_b[k] = (uint32_t)key;
        c_n[k] = cnt;
    }
    if (j < nq) {
        // (perf.clj:53: n * q as a double multiply, floored, capped at n - 1)
        const long long idx = min((long long)cnt - 1, (long long)floor((double)cnt * qs[j]));
        c_lat[(size_t)k * nq + j] = (int64_t)(ws[cap + p + (size_t)idx] ^ kPfSign);
    }
}

// h0 / h1 scanned: the l-th client cell (l = h1 at its head, below cap) from its key and its length
__global__ __launch_bounds__(kRvThreads) void k_pf_ratelist(size_t m, const uint64_t *ws, const uint32_t *h0,
                                                            const uint32_t *h1, const uint32_t *cpos, uint32_t cap,
                                                            uint32_t *r_f, uint32_t *r_t, uint32_t *r_b, uint32_t *r_n)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q >= m) return;
    const uint32_t l = h1[q];
    if (h1[q + 1] == l || l >= cap) return;
    const uint64_t key = ws[q];
    r_f[l] = (uint32_t)(key >> 35);
    r_t[l] = (uint32_t)(key >> 33) & 3;
    r_b[l] = (uint32_t)key;
    r_n[l] = cpos[h0[q] + 1] - (uint32_t)q;
}

// off[g] (g <= ng) = the first sorted position whose group (key >> shift) is at
// least g, from adjacent keys: position q writes the groups past its
// predecessor's up to its own (ng + 1 stores in all)
__global__ __launch_bounds__(kRvThreads) void k_pf_offsets(size_t m, const uint64_t *ws, int shift, uint32_t ng,
                                                           uint32_t *off)
{
    const size_t q = (size_t)blockIdx.x * kRvThreads + threadIdx.x;
    if (q > m) return;
    const uint64_t lo = q == 0 ? 0 : (ws[q - 1] >> shift) + 1;
    const uint64_t hi = q == m ? ng : min((uint64_t)ng, ws[q] >> shift);
    for (uint64_t g = lo; g <= hi; ++g) off[g] = (uint32_t)q;
}

// The phases' events: every way out of perf_run destroys them.
struct PhaseEvents {
    hipEvent_t e[HSC_PERF_NPHASE + 1] = {};
    int k = 0;
    ~PhaseEvents()
    {
        for (hipEvent_t x : e)
            if (x) (void)hipEventDestroy(x);
    }
    hipError_t mark(hipStream_t s)
    {
        hipError_t r = hipEventCreate(&e[k]);
        if (r == hipSuccess) r = hipEventRecord(e[k], s);
        ++k;
        return r;
    }
};

}  // namespace

void PerfBufs::release_all()
{
    t.release_all();
    DBuf *all[] = {&type, &f, &proc, &client, &time, &rows, &pay, &comp, &inv, &lat, &f0, &f1, &h0, &h1, &cpos,
                   &ct, &q, &c_f, &c_b, &c_n, &c_lat, &r_f, &r_t, &r_b, &r_n, &goff, &raw_op, &raw_off};
    for (DBuf *b : all) b->release();
}

#define CK(x)                          \
    do {                               \
        hipError_t e_ = (x);           \
        if (e_ != hipSuccess) return e_; \
    } while (0)

// A DBuf's first k elements into v (never left empty)
template <class T>
static hipError_t pf_fetch(std::vector<T> &v, const DBuf &b, size_t k, hipStream_t s)
{
    v.assign(std::max<size_t>(k, 1), 0);
    if (!k) return hipSuccess;
    return hipMemcpyAsync(v.data(), b.p, sizeof(T) * k, hipMemcpyDeviceToHost, s);
}

hipError_t perf_run(const PerfIn &in, PerfBufs &b, PerfOut &o, hipStream_t s)
{
    constexpr uint32_t cap = HSC_PERF_CELL_CAP;
    const size_t n = in.n;
    const uint32_t ng = in.nf * 4;
    o = PerfOut{};
    for (std::vector<uint32_t> *v : {&o.c_f, &o.c_b, &o.c_n, &o.r_f, &o.r_t, &o.r_b, &o.r_n, &o.raw_op})
        v->assign(1, 0);
    o.raw_off.assign((size_t)ng + 1, 0);
    o.counts.assign(ng, 0);
    o.c_lat.assign(1, 0);
    o.lat.assign(1, 0);
    o.comp.assign(1, 0);
    o.inv.assign(1, 0);
    if (!n) return hipSuccess;
    ResolveBufs &r = b.t;
    CK(b.type.ensure(n));
    CK(b.f.ensure(4 * n));
    CK(b.proc.ensure(4 * n));
    CK(b.client.ensure(n));
    CK(b.time.ensure(8 * n));
    CK(b.rows.ensure(8 * 2 * n));
    CK(b.pay.ensure(8 * n));
    CK(b.comp.ensure(4 * n));
    CK(b.inv.ensure(4 * n));
    CK(b.lat.ensure(8 * n));
    for (DBuf *x : {&b.f0, &b.f1, &b.h0, &b.h1, &b.cpos}) CK(x->ensure(4 * (n + 1)));
    CK(b.ct.ensure(8 * kPfWords));
    CK(b.q.ensure(8 * HSC_PERF_MAX_Q));
    const size_t lc = std::min<size_t>(n, cap);
    for (DBuf *x : {&b.c_f, &b.c_b, &b.c_n, &b.r_f, &b.r_t, &b.r_b, &b.r_n}) CK(x->ensure(4 * lc));
    CK(b.c_lat.ensure(8 * lc * std::max<size_t>(in.nq, 1)));
    CK(b.goff.ensure(4 * ((size_t)ng + 1)));
    CK(b.raw_off.ensure(4 * ((size_t)ng + 1)));
    // the sort's alternates and scratch (sort_rows2)
    CK(r.words2.ensure(8 * 2 * n));
    CK(r.pay2.ensure(8 * n));
    CK(r.gid.ensure(4 * n));
    CK(r.gid2.ensure(4 * n));
    CK(r.k0.ensure(8 * n));
    CK(r.k1.ensure(8 * n));
    CK(r.words_dev.ensure(256));
    CK(r.scratch.ensure(std::max(std::max(radix_scratch_bytes(n, 2), packed_scratch_bytes(n)),
                                 scan_scratch_bytes(n + 1) + 64)));
    const uint8_t *type = b.type.as<uint8_t>(), *client = b.client.as<uint8_t>();
    const uint32_t *f = b.f.as<uint32_t>();
    const int64_t *time = b.time.as<int64_t>();
    uint64_t *rows = b.rows.as<uint64_t>(), *pay = b.pay.as<uint64_t>();
    int32_t *comp = b.comp.as<int32_t>(), *inv = b.inv.as<int32_t>();
    int64_t *lat = b.lat.as<int64_t>();
    uint32_t *f0 = b.f0.as<uint32_t>(), *f1 = b.f1.as<uint32_t>(), *h0 = b.h0.as<uint32_t>(),
             *h1 = b.h1.as<uint32_t>(), *cpos = b.cpos.as<uint32_t>(), *scratch = r.scratch.as<uint32_t>();
    unsigned long long *ct = (unsigned long long *)b.ct.p;
    PhaseEvents ev;
    CK(ev.mark(s));
    // ---- rows
    CK(hipMemcpyAsync(b.type.p, in.type, n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(b.f.p, in.f, 4 * n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(b.proc.p, in.process, 4 * n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(b.client.p, in.client, n, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(b.time.p, in.time, 8 * n, hipMemcpyHostToDevice, s));
    if (in.nq) CK(hipMemcpyAsync(b.q.p, in.q, 8 * (size_t)in.nq, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(ct, 0, 8 * kPfWords, s));
    k_pf_rows<<<pf_blocks(n + 1), kRvThreads, 0, s>>>(n, type, f, b.proc.as<uint32_t>(), time, in.nf, in.q_dt,
                                                      in.r_dt, n, rows, pay, f1, ct);
    CK(hipGetLastError());
    unsigned long long hct[kPfWords] = {};
    CK(hipMemcpyAsync(hct, ct, 8 * kPfWords, hipMemcpyDeviceToHost, s));
    CK(ev.mark(s));
    CK(hipStreamSynchronize(s));
    if (hct[kPfBad]) {
        o.bad = true;
        return hipErrorInvalidValue;
    }
    o.invokes = hct[kPfInvokes];
    o.t_max = (int64_t)hct[kPfTmax];
    // ---- pair
    const uint64_t *ws, *ps;
    bool pk = false;
    CK(sort_rows2(n, n, r, rows, pay, &pk, &ws, &ps, s));
    o.sort_packed |= pk ? 1 : 0;
    k_pf_pair<<<pf_blocks(n + 1), kRvThreads, 0, s>>>(n, ws, ps, type, time, comp, inv, lat, f0, ct);
    CK(hipGetLastError());
    CK(scan_exclusive_u32(f0, n + 1, scratch, s));
    CK(scan_exclusive_u32(f1, n + 1, scratch, s));
    uint32_t np = 0, nc = 0;
    CK(hipMemcpyAsync(&np, f0 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(&nc, f1 + n, 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(hct, ct, 8 * kPfWords, hipMemcpyDeviceToHost, s));
    CK(ev.mark(s));
    CK(hipStreamSynchronize(s));
    o.paired = hct[kPfPaired];
    o.orphans = hct[kPfOrphans];
    // ---- latency cells
    uint32_t tot[2] = {0, 0};
    if (np) {
        k_pf_latrows<<<pf_blocks(n), kRvThreads, 0, s>>>(n, f0, f, time, lat, in.q_dt, n, rows, pay);
        CK(hipGetLastError());
        CK(sort_rows2(np, n, r, rows, pay, &pk, &ws, &ps, s));
        o.sort_packed |= pk ? 2 : 0;
        k_pf_heads<<<pf_blocks((size_t)np + 1), kRvThreads, 0, s>>>(np, ws, 0, h0, h0);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(h0, (size_t)np + 1, scratch, s));
        k_pf_cpos<<<pf_blocks((size_t)np + 1), kRvThreads, 0, s>>>(np, h0, cpos);
        CK(hipGetLastError());
        CK(hipMemcpyAsync(tot, h0 + np, 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        o.cells = tot[0];
        o.cells_listed = std::min(tot[0], cap);
        const uint32_t nq1 = std::max(in.nq, 1u);
        k_pf_quant<<<pf_blocks((size_t)o.cells_listed * nq1), kRvThreads, 0, s>>>(
            o.cells_listed, in.nq, nq1, b.q.as<double>(), ws, n, cpos, b.c_f.as<uint32_t>(), b.c_b.as<uint32_t>(),
            b.c_n.as<uint32_t>(), b.c_lat.as<int64_t>());
        CK(hipGetLastError());
        CK(pf_fetch(o.c_f, b.c_f, o.cells_listed, s));
        CK(pf_fetch(o.c_b, b.c_b, o.cells_listed, s));
        CK(pf_fetch(o.c_n, b.c_n, o.cells_listed, s));
        CK(pf_fetch(o.c_lat, b.c_lat, (size_t)o.cells_listed * in.nq, s));
    }
    CK(ev.mark(s));
    // ---- rate
    if (nc) {
        k_pf_raterows<<<pf_blocks(n), kRvThreads, 0, s>>>(n, f1, f, type, client, time, in.r_dt, n, rows, pay);
        CK(hipGetLastError());
        CK(sort_rows2(nc, n, r, rows, pay, &pk, &ws, &ps, s));
        o.sort_packed |= pk ? 4 : 0;
        k_pf_heads<<<pf_blocks((size_t)nc + 1), kRvThreads, 0, s>>>(nc, ws, 1ull << 32, h0, h1);
        CK(hipGetLastError());
        CK(scan_exclusive_u32(h0, (size_t)nc + 1, scratch, s));
        CK(scan_exclusive_u32(h1, (size_t)nc + 1, scratch, s));
        k_pf_cpos<<<pf_blocks((size_t)nc + 1), kRvThreads, 0, s>>>(nc, h0, cpos);
        CK(hipGetLastError());
        k_pf_ratelist<<<pf_blocks(nc), kRvThreads, 0, s>>>(nc, ws, h0, h1, cpos, cap, b.r_f.as<uint32_t>(),
                                                           b.r_t.as<uint32_t>(), b.r_b.as<uint32_t>(),
                                                           b.r_n.as<uint32_t>());
        CK(hipGetLastError());
        k_pf_offsets<<<pf_blocks((size_t)nc + 1), kRvThreads, 0, s>>>(nc, ws, 33, ng, b.goff.as<uint32_t>());
        CK(hipGetLastError());
        CK(hipMemcpyAsync(tot + 1, h1 + nc, 4, hipMemcpyDeviceToHost, s));
        std::vector<uint32_t> goff;
        CK(pf_fetch(goff, b.goff, (size_t)ng + 1, s));
        CK(hipStreamSynchronize(s));
        o.rate_cells = tot[1];
        o.rate_listed = std::min(tot[1], cap);
        for (uint32_t g = 0; g < ng; ++g) o.counts[g] = goff[g + 1] - goff[g];
        CK(pf_fetch(o.r_f, b.r_f, o.rate_listed, s));
        CK(pf_fetch(o.r_t, b.r_t, o.rate_listed, s));
        CK(pf_fetch(o.r_b, b.r_b, o.rate_listed, s));
        CK(pf_fetch(o.r_n, b.r_n, o.rate_listed, s));
    }
    CK(ev.mark(s));
    // ---- raw partition and the per-op arrays
    if (in.arrays) {
        o.n_arrays = n;
        o.n_raw = np;
        CK(pf_fetch(o.comp, b.comp, n, s));
        CK(pf_fetch(o.inv, b.inv, n, s));
        CK(pf_fetch(o.lat, b.lat, n, s));
        if (np) {
            k_pf_rawrows<<<pf_blocks(n), kRvThreads, 0, s>>>(n, f0, f, type, comp, n, rows, pay);
            CK(hipGetLastError());
            CK(sort_rows2(np, n, r, rows, pay, &pk, &ws, &ps, s));
            o.sort_packed |= pk ? 8 : 0;
            k_pf_offsets<<<pf_blocks((size_t)np + 1), kRvThreads, 0, s>>>(np, ws, 0, ng, b.raw_off.as<uint32_t>());
            CK(hipGetLastError());
            CK(pf_fetch(o.raw_off, b.raw_off, (size_t)ng + 1, s));
            // (the payloads are op indices below 2^31: the low words of the u64s)
            std::vector<uint64_t> tmp(np);
            CK(hipMemcpyAsync(tmp.data(), ps, 8 * (size_t)np, hipMemcpyDeviceToHost, s));
            CK(hipStreamSynchronize(s));
            o.raw_op.resize(np);
            for (uint32_t k = 0; k < np; ++k) o.raw_op[k] = (uint32_t)tmp[k];
        }
    }
    CK(ev.mark(s));
    CK(hipStreamSynchronize(s));
    for (int k = 0; k < HSC_PERF_NPHASE; ++k)
        if (hipEventElapsedTime(&o.phase_ms[k], ev.e[k], ev.e[k + 1]) != hipSuccess) o.phase_ms[k] = 0;
    return hipSuccess;
}
#undef CK

// load this file's code object now (see warm_graph)
hipError_t warm_perf()
{
    hipFuncAttributes a;
    return hipFuncGetAttributes(&a, (const void *)k_pf_rows);
}

}  // namespace hsc
