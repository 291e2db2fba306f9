// hsc_tally_host.cpp -- host side of hsc_tally_check and hsc_bank_check
// (DESIGN.md §5k): check the arguments, run hsc_tally.hip's passes on the
// context's stream inside one scoped event span and point the report at the
// context's host results.  Host code only, compiled as plain C++ like
// hsc_graph_host.cpp and hsc_linear_host.cpp.
#include "hsc_ctx.h"

#include <cstring>

extern "C" int hsc_tally_check(hsc_ctx *c, const hsc_tally_in *in, unsigned flags, hsc_tally_report *out)
{
    if (!c || !in || !out) return HSC_EINVAL;
    if (flags & ~HSC_TALLY_MULTISET) return HSC_EINVAL;
    if ((in->n_attempt && !in->attempt) || (in->n_ack && !in->ack) || (in->n_seen && !in->seen)) return HSC_EINVAL;
    // (each length first: their sum must not wrap)
    const size_t kMax = 0x7FFFFFFFull;
    if (in->n_attempt > kMax || in->n_ack > kMax || in->n_seen > kMax ||
        in->n_attempt + in->n_ack + in->n_seen > kMax)
        return HSC_EINVAL;
    if (c->host_only) return HSC_EDEVICE;
    MuGuard g_(c);
    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    TallyOut &o = c->tally_out;
    const TallyIn ti{in->n_attempt, in->n_ack, in->n_seen, in->attempt, in->ack, in->seen,
                     (flags & HSC_TALLY_MULTISET) != 0};
    EventSpan t;
    HIPCHK(c, t.begin(s));
    HIPCHK(c, tally_run(ti, c->tally, o, s));
    HIPCHK(c, t.end(s));
    HIPCHK(c, hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->attempts = o.total[0];
    out->acks = o.total[1];
    out->seen = o.total[2];
    out->distinct = o.distinct;
    for (int k = 0; k < HSC_TALLY_NCLASS; ++k) {
        hsc_tally_class &q = out->cls[k];
        q.count = o.count[k];
        q.distinct = o.ndistinct[k];
        q.runs = o.runs[k];
        q.n_listed = o.n_listed[k];
        q.lo = o.lo[k].data();
        q.hi = o.hi[k].data();
        q.mult = o.mult[k].data();
    }
    out->valid = !o.count[HSC_TALLY_LOST] && !o.count[HSC_TALLY_UNEXPECTED];
    out->sort_packed = o.sort_packed;
    out->ms = t.ms();
    return HSC_OK;
}

extern "C" int hsc_bank_check(hsc_ctx *c, const hsc_bank_in *in, hsc_bank_report *out)
{
    if (!c || !in || !out) return HSC_EINVAL;
    const size_t nr = in->n_reads;
    if (nr > 0x7FFFFFFFull || (nr && !in->off)) return HSC_EINVAL;
    if (nr) {
        if (in->off[0] != 0) return HSC_EINVAL;
        for (size_t i = 0; i < nr; ++i)
            if (in->off[i + 1] < in->off[i]) return HSC_EINVAL;
        if (in->off[nr] > 0xFFFFFFFFull || (in->off[nr] && !in->balance)) return HSC_EINVAL;
    }
    if (c->host_only) return HSC_EDEVICE;
    MuGuard g_(c);
    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    BankOut &o = c->bank_out;
    const BankIn bi{nr, in->off, in->balance, in->n, in->total};
    EventSpan t;
    HIPCHK(c, t.begin(s));
    HIPCHK(c, bank_run(bi, c->bank, o, s));
    HIPCHK(c, t.end(s));
    HIPCHK(c, hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->n_reads = nr;
    out->bad = o.bad;
    out->wrong_n = o.wrong_n;
    out->wrong_total = o.wrong_total;
    out->reads_with_negative = o.with_negative;
    out->valid = o.bad == 0;
    out->kind = o.kind.data();
    out->found = o.found.data();
    out->negatives = o.neg.data();
    out->n_listed = o.n_listed;
    out->listed_read = o.listed.data();
    out->ms = t.ms();
    return HSC_OK;
}
