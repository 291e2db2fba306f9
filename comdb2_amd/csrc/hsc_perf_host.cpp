// hsc_perf_host.cpp -- host side of hsc_perf_check: check the
// arguments, run hsc_perf.hip's passes on the context's stream inside one
// scoped event span and point the report at the context's host results.  Host
// code only, compiled as plain C++ like hsc_tally_host.cpp.
#include "hsc_ctx.h"

#include <cmath>
#include <cstring>

extern "C" int hsc_perf_check(hsc_ctx *c, const hsc_perf_in *in, unsigned flags, hsc_perf_report *out)
{
    if (!c || !in || !out) return HSC_EINVAL;
    if (flags & ~HSC_PERF_ARRAYS) return HSC_EINVAL;
    if (in->n && (!in->type || !in->f || !in->process || !in->client || !in->time)) return HSC_EINVAL;
    if (in->n > 0x7FFFFFFFull) return HSC_EINVAL;
    if (!in->nf || in->nf > HSC_PERF_MAX_F) return HSC_EINVAL;
    if (in->nq > HSC_PERF_MAX_Q || (in->nq && !in->q)) return HSC_EINVAL;
    for (uint32_t j = 0; j < in->nq; ++j)
        if (!(in->q[j] >= 0.0 && in->q[j] <= 1.0)) return HSC_EINVAL;  // (a NaN fails both)
    if (!(in->q_dt > 0.0) || !(in->r_dt > 0.0) || !std::isfinite(in->q_dt) || !std::isfinite(in->r_dt))
        return HSC_EINVAL;
    if (c->host_only) return HSC_EDEVICE;
    MuGuard g_(c);
    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    PerfOut &o = c->perf_out;
    const PerfIn pi{in->n, in->type, in->f, in->process, in->client, in->time, in->nf, in->nq, in->q,
                    in->q_dt, in->r_dt, (flags & HSC_PERF_ARRAYS) != 0};
    EventSpan t;
    HIPCHK(c, t.begin(s));
    const hipError_t e = perf_run(pi, c->perf, o, s);
    if (e == hipErrorInvalidValue && o.bad) return HSC_EINVAL;  // the device's input checks
    HIPCHK(c, e);
    HIPCHK(c, t.end(s));
    HIPCHK(c, hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->n = in->n;
    out->invokes = o.invokes;
    out->paired = o.paired;
    out->unpaired = o.invokes - o.paired;
    out->orphans = o.orphans;
    out->t_max = o.t_max;
    out->cells = o.cells;
    out->rate_cells = o.rate_cells;
    out->cells_listed = o.cells_listed;
    out->rate_listed = o.rate_listed;
    out->cell_f = o.c_f.data();
    out->cell_bucket = o.c_b.data();
    out->cell_count = o.c_n.data();
    out->cell_lat = o.c_lat.data();
    out->rate_f = o.r_f.data();
    out->rate_type = o.r_t.data();
    out->rate_bucket = o.r_b.data();
    out->rate_count = o.r_n.data();
    out->counts = o.counts.data();
    out->n_arrays = o.n_arrays;
    out->completion_of = o.comp.data();
    out->invoke_of = o.inv.data();
    out->latency = o.lat.data();
    out->n_raw = o.n_raw;
    out->raw_op = o.raw_op.data();
    out->raw_off = o.raw_off.data();
    out->sort_packed = o.sort_packed;
    out->ms = t.ms();
    for (int k = 0; k < HSC_PERF_NPHASE; ++k) out->phase_ms[k] = o.phase_ms[k];
    return HSC_OK;
}
