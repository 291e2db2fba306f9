// hsc_linear_host.cpp -- host side of hsc_linear_check: split
// a register history by key, order each key's calls and returns, give the ops
// slots and the values dense ids, write the keys' event programs, upload them
// in one copy, run hsc_linear.hip's search (one workgroup per key) on the
// context's stream and turn its result words into the report.  Host code only,
// compiled as plain C++ like hsc_graph_host.cpp.
#include "hsc_ctx.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

struct KeyEvent {
    uint64_t pos;
    uint32_t op;
    uint8_t ret;
    bool operator<(const KeyEvent &o) const
    {
        if (pos != o.pos) return pos < o.pos;
        if (ret != o.ret) return ret < o.ret;  // calls before returns: equal times overlap
        return op < o.op;
    }
};

}  // namespace

extern "C" int hsc_linear_check(hsc_ctx *c, const hsc_lin_ops *ops, hsc_lin_report *out)
{
    if (!c || !ops || !out) return HSC_EINVAL;
    const size_t n = ops->nops;
    const uint32_t nk = ops->nkeys;
    if (n && (!ops->key || !ops->f || !ops->a || !ops->b || !ops->invoke || !ops->complete)) return HSC_EINVAL;
    if (n > 0x3FFFFFFFull) return HSC_EINVAL;
    if (c->host_only) return HSC_EDEVICE;
    MuGuard g_(c);
    (void)hipSetDevice(c->device);
    for (size_t i = 0; i < n; ++i) {
        if (ops->key[i] >= nk) return ctx_fail(c, HSC_EINVAL, "register history: an op names a key >= nkeys");
        if (ops->f[i] > HSC_LIN_CAS) return ctx_fail(c, HSC_EINVAL, "register history: an unknown f");
        if (ops->complete[i] != HSC_RT_OPEN && ops->invoke[i] >= ops->complete[i])
            return ctx_fail(c, HSC_EINVAL, "register history: a closed op completes at or before its invoke");
    }
    LinearOut &o = c->linear_out;
    o.verdict.assign(std::max<uint32_t>(nk, 1), HSC_LIN_OK);
    o.cause.assign(std::max<uint32_t>(nk, 1), 0);
    o.fail_op.assign(std::max<uint32_t>(nk, 1), 0xFFFFFFFFu);
    o.prev_ok.assign(std::max<uint32_t>(nk, 1), 0xFFFFFFFFu);
    o.peak.assign(std::max<uint32_t>(nk, 1), 1);
    o.final_n.assign(std::max<uint32_t>(nk, 1), 1);
    o.state_off.assign((size_t)nk + 1, 0);
    o.state_val.clear();
    memset(out, 0, sizeof *out);
    uint64_t dropped = 0;

    // the ops of each key, in op order
    std::vector<size_t> koff((size_t)nk + 1, 0);
    for (size_t i = 0; i < n; ++i) koff[ops->key[i] + 1]++;
    for (uint32_t k = 0; k < nk; ++k) koff[k + 1] += koff[k];
    std::vector<uint32_t> kop(std::max<size_t>(n, 1));
    {
        std::vector<size_t> at(koff.begin(), koff.end() - 1);
        for (size_t i = 0; i < n; ++i) kop[at[ops->key[i]]++] = (uint32_t)i;
    }

    // the event programs of the keys to launch
    std::vector<LinEvent> prog;
    std::vector<LinKey> keys;
    std::vector<uint32_t> key_of;        // launched key -> key
    std::vector<int64_t> vals_all;       // the launched keys' values, ascending per key: id = 1 + the index
    std::vector<size_t> vals_off;        // launched key -> its values in vals_all
    prog.reserve(2 * n);
    std::vector<KeyEvent> evs;
    std::vector<int64_t> vals;
    uint32_t seen_total = 0;
    for (uint32_t k = 0; k < nk; ++k) {
        evs.clear();
        vals.clear();
        const int64_t init = ops->init ? ops->init[k] : HSC_LIN_NIL;
        if (init != HSC_LIN_NIL) vals.push_back(init);
        for (size_t q = koff[k]; q < koff[k + 1]; ++q) {
            const uint32_t i = kop[q];
            const bool open = ops->complete[i] == HSC_RT_OPEN;
            if (open && ops->f[i] == HSC_LIN_READ) {  // changes no state, nothing waits for it
                ++dropped;
                continue;
            }
            evs.push_back({ops->invoke[i], i, 0});
            if (!open) evs.push_back({ops->complete[i], i, 1});
            if (ops->a[i] != HSC_LIN_NIL) vals.push_back(ops->a[i]);
            if (ops->f[i] == HSC_LIN_CAS && ops->b[i] != HSC_LIN_NIL) vals.push_back(ops->b[i]);
        }
        if (evs.empty()) continue;
        std::sort(evs.begin(), evs.end());
        std::sort(vals.begin(), vals.end());
        vals.erase(std::unique(vals.begin(), vals.end()), vals.end());
        auto id_of = [&](int64_t v) -> uint32_t {
            return v == HSC_LIN_NIL ? 0u : 1u + (uint32_t)(std::lower_bound(vals.begin(), vals.end(), v) - vals.begin());
        };
        // the lowest free slot at a call, freed at the return; open ops keep theirs
        const size_t ev0 = prog.size();
        uint32_t used = 0;
        bool fits = true;
        // (slot of an op in flight: ops of one key return in event order, found by op index)
        std::vector<std::pair<uint32_t, uint32_t>> inflight;  // (op, slot), few
        for (const KeyEvent &e : evs) {
            if (!e.ret) {
                if (used == 0xFFFFFFFFu) {
                    fits = false;
                    break;
                }
                const uint32_t slot = (uint32_t)__builtin_ctz(~used);
                used |= 1u << slot;
                if (ops->complete[e.op] != HSC_RT_OPEN) inflight.push_back({e.op, slot});
                const uint32_t f = ops->f[e.op];
                prog.push_back({slot << 1 | f << 8, id_of(ops->a[e.op]), f == HSC_LIN_CAS ? id_of(ops->b[e.op]) : 0u, e.op});
            } else {
                size_t p = 0;
                while (inflight[p].first != e.op) ++p;
                const uint32_t slot = inflight[p].second;
                inflight[p] = inflight.back();
                inflight.pop_back();
                used &= ~(1u << slot);
                prog.push_back({1u | slot << 1, 0u, 0u, e.op});
            }
        }
        if (!fits) {  // a 33rd pending op: not launched
            prog.resize(ev0);
            o.verdict[k] = HSC_LIN_UNKNOWN;
            o.cause[k] = HSC_LIN_CAUSE_SLOTS;
            o.peak[k] = o.final_n[k] = 0;
            continue;
        }
        keys.push_back({(uint32_t)ev0, (uint32_t)(prog.size() - ev0), id_of(init), seen_total});
        key_of.push_back(k);
        vals_off.push_back(vals_all.size());
        vals_all.insert(vals_all.end(), vals.begin(), vals.end());
        seen_total += (uint32_t)vals.size() + 1;
    }
    vals_off.push_back(vals_all.size());

    const uint32_t nl = (uint32_t)keys.size();
    float ms = 0;
    uint64_t expanded = 0;
    if (nl) {
        hipStream_t s = c->stream;
        // events | keys | results | seen
        const size_t b_ev = sizeof(LinEvent) * prog.size(), b_key = sizeof(LinKey) * (size_t)nl,
                     b_res = sizeof(LinResult) * (size_t)nl, b_seen = ((size_t)seen_total + 15) & ~(size_t)15;
        std::vector<uint8_t> up(b_ev + b_key), down(b_res + b_seen);
        memcpy(up.data(), prog.data(), b_ev);
        memcpy(up.data() + b_ev, keys.data(), b_key);
        HIPCHK(c, c->linear.arena.ensure(b_ev + b_key + b_res + b_seen));
        uint8_t *d = c->linear.arena.as<uint8_t>();
        EventSpan t;
        HIPCHK(c, t.begin(s));
        HIPCHK(c, hipMemcpyAsync(d, up.data(), up.size(), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipMemsetAsync(d + up.size(), 0, down.size(), s));
        HIPCHK(c, linear_search((const LinEvent *)d, (const LinKey *)(d + b_ev), nl, (LinResult *)(d + up.size()),
                                d + up.size() + b_res, s));
        HIPCHK(c, t.end(s));
        HIPCHK(c, hipMemcpyAsync(down.data(), d + up.size(), down.size(), hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        ms = t.ms();
        const LinResult *res = (const LinResult *)down.data();
        const uint8_t *seen = down.data() + b_res;
        for (uint32_t l = 0; l < nl; ++l) {
            const uint32_t k = key_of[l];
            const LinResult &r = res[l];
            o.verdict[k] = (uint8_t)r.verdict;
            o.cause[k] = (uint8_t)r.cause;
            o.peak[k] = r.peak;
            o.final_n[k] = r.final_n;
            expanded += (uint64_t)r.expanded_hi << 32 | r.expanded_lo;
            if (r.verdict != HSC_LIN_BAD || r.fail_ev >= keys[l].nev) continue;
            const LinEvent *pe = prog.data() + keys[l].ev_off;
            o.fail_op[k] = pe[r.fail_ev].op;
            for (uint32_t e = r.fail_ev; e-- > 0;)
                if (pe[e].w & 1u) {
                    o.prev_ok[k] = pe[e].op;
                    break;
                }
        }
        // the states of the BAD keys' sets, in key order
        std::vector<uint32_t> launch_of(nk, 0xFFFFFFFFu);
        for (uint32_t l = 0; l < nl; ++l) launch_of[key_of[l]] = l;
        for (uint32_t k = 0; k < nk; ++k) {
            o.state_off[k] = o.state_val.size();
            const uint32_t l = launch_of[k];
            if (l == 0xFFFFFFFFu || o.verdict[k] != HSC_LIN_BAD) continue;
            const uint8_t *sk = seen + keys[l].seen_off;
            const size_t nv = vals_off[l + 1] - vals_off[l];
            if (sk[0]) o.state_val.push_back(HSC_LIN_NIL);
            for (size_t j = 0; j < nv; ++j)
                if (sk[j + 1]) o.state_val.push_back(vals_all[vals_off[l] + j]);
        }
        o.state_off[nk] = o.state_val.size();
    }
    static const int64_t kNoVal[1] = {0};
    out->nkeys = nk;
    out->verdict = o.verdict.data();
    out->cause = o.cause.data();
    out->fail_op = o.fail_op.data();
    out->prev_ok = o.prev_ok.data();
    out->peak_configs = o.peak.data();
    out->final_configs = o.final_n.data();
    out->state_off = o.state_off.data();
    out->state_val = o.state_val.empty() ? kNoVal : o.state_val.data();
    for (uint32_t k = 0; k < nk; ++k) {
        out->bad += o.verdict[k] == HSC_LIN_BAD;
        out->unknown += o.verdict[k] == HSC_LIN_UNKNOWN;
    }
    out->events = prog.size();
    out->expanded = expanded;
    out->dropped_open_reads = dropped;
    out->ms = ms;
    return HSC_OK;
}
