// hsc_count_host.cpp -- host side of hsc_counter_check and hsc_queue_check
// (DESIGN.md §5m): check the arguments -- the keys, types and fs too, so no
// kernel ever indexes a per-key array out of range -- run hsc_count.hip's
// passes on the context's stream inside one scoped event span and point the
// report at the context's host results.  Host code only, compiled as plain C++
// like hsc_tally_host.cpp and hsc_perf_host.cpp.
#include "hsc_ctx.h"

#include <cstring>

namespace {

// every key below nkeys (key null: nkeys must be 1), every code at most max_code
bool rows_ok(size_t n, const uint32_t *key, uint32_t nkeys, const uint8_t *a, uint8_t max_a, const uint8_t *b,
             uint8_t max_b)
{
    if (!key && nkeys != 1) return false;
    for (size_t i = 0; i < n; ++i) {
        if (key && key[i] >= nkeys) return false;
        if (a[i] > max_a) return false;
        if (b && b[i] > max_b) return false;
    }
    return true;
}

}  // namespace

extern "C" int hsc_counter_check(hsc_ctx *c, const hsc_counter_in *in, hsc_counter_report *out)
{
    if (!c || !in || !out) return HSC_EINVAL;
    if (in->n && (!in->type || !in->f || !in->process || !in->value)) return HSC_EINVAL;
    if (in->n > 0x7FFFFFFFull) return HSC_EINVAL;
    if (!in->nkeys) return HSC_EINVAL;
    if (in->n && !rows_ok(in->n, in->key, in->nkeys, in->type, HSC_OP_INFO, in->f, HSC_CNT_OTHER)) return HSC_EINVAL;
    if (c->host_only) return HSC_EDEVICE;
    MuGuard g_(c);
    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    CounterOut &o = c->counter_out;
    const CounterIn ci{in->n, in->type, in->f, in->process, in->value, in->key, in->nkeys};
    EventSpan t;
    HIPCHK(c, t.begin(s));
    HIPCHK(c, counter_run(ci, c->count, o, s));
    HIPCHK(c, t.end(s));
    HIPCHK(c, hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->nkeys = in->nkeys;
    out->bad = o.bad;
    out->unknown = o.unknown;
    out->verdict = o.verdict.data();
    out->malformed_op = o.mal_op.data();
    out->malformed_kind = o.mal_kind.data();
    out->read_off = o.read_off.data();
    out->reads = o.reads;
    out->bad_reads = o.bad_reads;
    out->lower = o.lower.data();
    out->value = o.value.data();
    out->upper = o.upper.data();
    out->read_op = o.read_op.data();
    out->errors = o.errors.data();
    out->n_listed = o.n_listed;
    out->listed_read = o.listed.data();
    out->sort_packed = o.sort_packed;
    out->ms = t.ms();
    return HSC_OK;
}

extern "C" int hsc_queue_check(hsc_ctx *c, const hsc_queue_in *in, unsigned flags, hsc_queue_report *out)
{
    if (!c || !in || !out) return HSC_EINVAL;
    if (flags & ~(HSC_QUEUE_FIFO | HSC_QUEUE_FINAL)) return HSC_EINVAL;
    if (in->n && (!in->f || !in->value)) return HSC_EINVAL;
    if (in->n > 0x7FFFFFFFull) return HSC_EINVAL;
    if (!in->nkeys) return HSC_EINVAL;
    if (in->n && !rows_ok(in->n, in->key, in->nkeys, in->f, HSC_Q_DEQUEUE, nullptr, 0)) return HSC_EINVAL;
    if (c->host_only) return HSC_EDEVICE;
    MuGuard g_(c);
    (void)hipSetDevice(c->device);
    hipStream_t s = c->stream;
    QueueOut &o = c->queue_out;
    const QueueIn qi{in->n, in->f, in->value, in->key, in->nkeys, (flags & HSC_QUEUE_FIFO) != 0,
                     (flags & HSC_QUEUE_FINAL) != 0};
    EventSpan t;
    HIPCHK(c, t.begin(s));
    HIPCHK(c, queue_run(qi, c->count, o, s));
    HIPCHK(c, t.end(s));
    HIPCHK(c, hipStreamSynchronize(s));
    memset(out, 0, sizeof *out);
    out->nkeys = in->nkeys;
    out->bad = o.bad;
    out->verdict = o.verdict.data();
    out->error_row = o.error_row.data();
    out->error_kind = o.kind.data();
    out->final_len = o.final_len.data();
    out->final_off = o.final_off.data();
    out->n_final = o.n_final;
    out->final_val = o.final_val.data();
    out->final_mult = o.final_mult.data();
    out->sort_packed = o.sort_packed;
    out->ms = t.ms();
    return HSC_OK;
}
