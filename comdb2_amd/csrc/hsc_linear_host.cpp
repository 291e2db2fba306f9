// hsc_linear_host.cpp -- host side of hsc_linear_check and
// hsc_linear_check_wide: split a register history by key, order
// each key's calls and returns, give the ops slots and the values dense ids,
// write the keys' event programs, upload them in one copy, run the search (one
// workgroup per key; hsc_linear.hip, and hsc_linear_wide.hip for the keys whose
// search leaves LDS) on the context's stream and turn its result words into
// the report.  Host code only, compiled as plain C++ like hsc_graph_host.cpp.
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

// the ops of each key, in op order
struct OpsIndex {
    std::vector<size_t> koff;
    std::vector<uint32_t> kop;
};

// the event programs of one tier's launch
struct Programs {
    std::vector<LinEvent> prog;
    std::vector<LinKey> keys;
    std::vector<uint32_t> key_of;   // launched key -> key
    std::vector<int64_t> vals_all;  // the launched keys' values, ascending per key: id = 1 + the index
    std::vector<size_t> vals_off;   // launched key -> its values in vals_all
    uint32_t seen_total = 0;
};

const char *invalid_ops(const hsc_lin_ops *ops)
{
    for (size_t i = 0; i < ops->nops; ++i) {
        if (ops->key[i] >= ops->nkeys) return "register history: an op names a key >= nkeys";
        if (ops->f[i] > HSC_LIN_CAS) return "register history: an unknown f";
        if (ops->complete[i] != HSC_RT_OPEN && ops->invoke[i] >= ops->complete[i])
            return "register history: a closed op completes at or before its invoke";
    }
    return nullptr;
}

// every key as one without events: OK, one configuration
void reset_key(LinearOut &o, uint32_t k)
{
    o.verdict[k] = HSC_LIN_OK;
    o.cause[k] = 0;
    o.fail_op[k] = o.prev_ok[k] = 0xFFFFFFFFu;
    o.peak[k] = o.final_n[k] = 1;
    o.events[k] = 0;
    o.expanded[k] = 0;
    o.states[k].clear();
}

void reset_out(LinearOut &o, uint32_t nk)
{
    const uint32_t n1 = std::max<uint32_t>(nk, 1);
    o.verdict.assign(n1, HSC_LIN_OK);
    o.cause.assign(n1, 0);
    o.fail_op.assign(n1, 0xFFFFFFFFu);
    o.prev_ok.assign(n1, 0xFFFFFFFFu);
    o.peak.assign(n1, 1);
    o.final_n.assign(n1, 1);
    o.events.assign(n1, 0);
    o.expanded.assign(n1, 0);
    o.states.assign(n1, {});
    o.tier.assign(n1, 0);
    o.state_off.assign((size_t)nk + 1, 0);
    o.state_val.clear();
}

void index_ops(const hsc_lin_ops *ops, OpsIndex &ix)
{
    const size_t n = ops->nops;
    const uint32_t nk = ops->nkeys;
    ix.koff.assign((size_t)nk + 1, 0);
    for (size_t i = 0; i < n; ++i) ix.koff[ops->key[i] + 1]++;
    for (uint32_t k = 0; k < nk; ++k) ix.koff[k + 1] += ix.koff[k];
    ix.kop.resize(std::max<size_t>(n, 1));
    std::vector<size_t> at(ix.koff.begin(), ix.koff.end() - 1);
    for (size_t i = 0; i < n; ++i) ix.kop[at[ops->key[i]]++] = (uint32_t)i;
}

// The event programs of the keys with pick[k] (NULL: every key) at `slots`
// pending ops (<= 64; the event word holds 6 slot bits) and at most
// `max_states` distinct non-nil values (0: no limit).  A key that needs more
// is UNKNOWN with the cause and is not launched.  dropped: counts the open
// reads left out, when given.
void build_programs(const hsc_lin_ops *ops, const OpsIndex &ix, const uint8_t *pick, uint32_t slots,
                    uint32_t max_states, LinearOut &o, uint64_t *dropped, Programs &p)
{
    const uint32_t nk = ops->nkeys;
    const uint64_t all_used = slots >= 64 ? ~0ull : (1ull << slots) - 1;
    p.prog.reserve(2 * ops->nops);
    std::vector<KeyEvent> evs;
    std::vector<int64_t> vals;
    for (uint32_t k = 0; k < nk; ++k) {
        if (pick && !pick[k]) continue;
        reset_key(o, k);
        evs.clear();
        vals.clear();
        const int64_t init = ops->init ? ops->init[k] : HSC_LIN_NIL;
        if (init != HSC_LIN_NIL) vals.push_back(init);
        for (size_t q = ix.koff[k]; q < ix.koff[k + 1]; ++q) {
            const uint32_t i = ix.kop[q];
            const bool open = ops->complete[i] == HSC_RT_OPEN;
            if (open && ops->f[i] == HSC_LIN_READ) {  // changes no state, nothing waits for it
                if (dropped) ++*dropped;
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
        const size_t ev0 = p.prog.size();
        uint64_t used = 0;
        bool fits = true;
        // (slot of an op in flight: ops of one key return in event order, found by op index)
        std::vector<std::pair<uint32_t, uint32_t>> inflight;  // (op, slot), few
        for (const KeyEvent &e : evs) {
            if (!e.ret) {
                if (used == all_used) {
                    fits = false;
                    break;
                }
                const uint32_t slot = (uint32_t)__builtin_ctzll(~used);
                used |= 1ull << slot;
                if (ops->complete[e.op] != HSC_RT_OPEN) inflight.push_back({e.op, slot});
                const uint32_t f = ops->f[e.op];
                p.prog.push_back({slot << 1 | f << 8, id_of(ops->a[e.op]), f == HSC_LIN_CAS ? id_of(ops->b[e.op]) : 0u, e.op});
            } else {
                size_t q = 0;
                while (inflight[q].first != e.op) ++q;
                const uint32_t slot = inflight[q].second;
                inflight[q] = inflight.back();
                inflight.pop_back();
                used &= ~(1ull << slot);
                p.prog.push_back({1u | slot << 1, 0u, 0u, e.op});
            }
        }
        const bool states_fit = !max_states || vals.size() <= max_states;
        if (!fits || !states_fit) {  // one pending op, or one value, too many: not launched
            p.prog.resize(ev0);
            o.verdict[k] = HSC_LIN_UNKNOWN;
            o.cause[k] = !fits ? HSC_LIN_CAUSE_SLOTS : HSC_LIN_CAUSE_STATES;
            o.peak[k] = o.final_n[k] = 0;
            continue;
        }
        p.keys.push_back({(uint32_t)ev0, (uint32_t)(p.prog.size() - ev0), id_of(init), p.seen_total});
        p.key_of.push_back(k);
        p.vals_off.push_back(p.vals_all.size());
        p.vals_all.insert(p.vals_all.end(), vals.begin(), vals.end());
        p.seen_total += (uint32_t)vals.size() + 1;
    }
    p.vals_off.push_back(p.vals_all.size());
}

// Upload p's programs and key table, search (wide NULL: the LDS tier, one
// launch; else the wide tier, per_round keys a launch), read the result words
// and state flags back once and write the launched keys' fields into o.
int run_tier(hsc_ctx *c, const Programs &p, const LinWideLimits *wide, uint32_t per_round, LinearOut &o, float *ms,
             uint32_t *rounds)
{
    const uint32_t nl = (uint32_t)p.keys.size();
    if (!nl) return HSC_OK;
    hipStream_t s = c->stream;
    // events | keys | results | seen
    const size_t b_ev = sizeof(LinEvent) * p.prog.size(), b_key = sizeof(LinKey) * (size_t)nl,
                 b_res = sizeof(LinResult) * (size_t)nl, b_seen = ((size_t)p.seen_total + 15) & ~(size_t)15;
    std::vector<uint8_t> up(b_ev + b_key), down(b_res + b_seen);
    memcpy(up.data(), p.prog.data(), b_ev);
    memcpy(up.data() + b_ev, p.keys.data(), b_key);
    HIPCHK(c, c->linear.arena.ensure(b_ev + b_key + b_res + b_seen));
    if (wide) HIPCHK(c, c->linear.wide.ensure((size_t)std::min(per_round, nl) * 32 * wide->max_configs));
    uint8_t *d = c->linear.arena.as<uint8_t>();
    const LinEvent *d_prog = (const LinEvent *)d;
    const LinKey *d_keys = (const LinKey *)(d + b_ev);
    LinResult *d_res = (LinResult *)(d + up.size());
    uint8_t *d_seen = d + up.size() + b_res;
    EventSpan t;
    HIPCHK(c, t.begin(s));
    HIPCHK(c, hipMemcpyAsync(d, up.data(), up.size(), hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemsetAsync(d + up.size(), 0, down.size(), s));
    if (!wide) {
        HIPCHK(c, linear_search(d_prog, d_keys, nl, d_res, d_seen, s));
    } else {
        for (uint32_t l0 = 0; l0 < nl; l0 += per_round, ++*rounds)
            HIPCHK(c, linear_search_wide(d_prog, d_keys + l0, std::min(per_round, nl - l0), d_res + l0, d_seen,
                                         c->linear.wide.as<uint64_t>(), *wide, s));
    }
    HIPCHK(c, t.end(s));
    HIPCHK(c, hipMemcpyAsync(down.data(), d + up.size(), down.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *ms = t.ms();
    const LinResult *res = (const LinResult *)down.data();
    const uint8_t *seen = down.data() + b_res;
    for (uint32_t l = 0; l < nl; ++l) {
        const uint32_t k = p.key_of[l];
        const LinResult &r = res[l];
        o.verdict[k] = (uint8_t)r.verdict;
        o.cause[k] = (uint8_t)r.cause;
        o.peak[k] = r.peak;
        o.final_n[k] = r.final_n;
        o.events[k] = p.keys[l].nev;
        o.expanded[k] = (uint64_t)r.expanded_hi << 32 | r.expanded_lo;
        if (r.verdict != HSC_LIN_BAD || r.fail_ev >= p.keys[l].nev) continue;
        const LinEvent *pe = p.prog.data() + p.keys[l].ev_off;
        o.fail_op[k] = pe[r.fail_ev].op;
        for (uint32_t e = r.fail_ev; e-- > 0;)
            if (pe[e].w & 1u) {
                o.prev_ok[k] = pe[e].op;
                break;
            }
        // the states of the BAD key's set
        const uint8_t *sk = seen + p.keys[l].seen_off;
        const size_t nv = p.vals_off[l + 1] - p.vals_off[l];
        if (sk[0]) o.states[k].push_back(HSC_LIN_NIL);
        for (size_t j = 0; j < nv; ++j)
            if (sk[j + 1]) o.states[k].push_back(p.vals_all[p.vals_off[l] + j]);
    }
    return HSC_OK;
}

void fill_report(LinearOut &o, uint32_t nk, uint64_t dropped, float ms, hsc_lin_report *out)
{
    static const int64_t kNoVal[1] = {0};
    memset(out, 0, sizeof *out);
    o.state_val.clear();
    for (uint32_t k = 0; k < nk; ++k) {
        o.state_off[k] = o.state_val.size();
        if (o.verdict[k] == HSC_LIN_BAD) o.state_val.insert(o.state_val.end(), o.states[k].begin(), o.states[k].end());
        out->bad += o.verdict[k] == HSC_LIN_BAD;
        out->unknown += o.verdict[k] == HSC_LIN_UNKNOWN;
        out->events += o.events[k];
        out->expanded += o.expanded[k];
    }
    o.state_off[nk] = o.state_val.size();
    out->nkeys = nk;
    out->verdict = o.verdict.data();
    out->cause = o.cause.data();
    out->fail_op = o.fail_op.data();
    out->prev_ok = o.prev_ok.data();
    out->peak_configs = o.peak.data();
    out->final_configs = o.final_n.data();
    out->state_off = o.state_off.data();
    out->state_val = o.state_val.empty() ? kNoVal : o.state_val.data();
    out->dropped_open_reads = dropped;
    out->ms = ms;
}

bool ops_null(const hsc_lin_ops *ops)
{
    return ops->nops && (!ops->key || !ops->f || !ops->a || !ops->b || !ops->invoke || !ops->complete);
}

}  // namespace

extern "C" int hsc_linear_check(hsc_ctx *c, const hsc_lin_ops *ops, hsc_lin_report *out)
{
    if (!c || !ops || !out) return HSC_EINVAL;
    if (ops_null(ops)) return HSC_EINVAL;
    if (ops->nops > 0x3FFFFFFFull) return HSC_EINVAL;
    if (c->host_only) return HSC_EDEVICE;
    MuGuard g_(c);
    (void)hipSetDevice(c->device);
    if (const char *why = invalid_ops(ops)) return ctx_fail(c, HSC_EINVAL, why);
    LinearOut &o = c->linear_out;
    reset_out(o, ops->nkeys);
    memset(out, 0, sizeof *out);
    OpsIndex ix;
    index_ops(ops, ix);
    Programs p;
    uint64_t dropped = 0;
    build_programs(ops, ix, nullptr, kLinSlots, 0, o, &dropped, p);
    float ms = 0;
    HIPCHK_RC(c, run_tier(c, p, nullptr, 0, o, &ms, nullptr));
    fill_report(o, ops->nkeys, dropped, ms, out);
    return HSC_OK;
}

extern "C" int hsc_linear_check_wide(hsc_ctx *c, const hsc_lin_ops *ops, const hsc_lin_wide_limits *limits,
                                     hsc_lin_wide_report *out)
{
    if (!c || !ops || !out) return HSC_EINVAL;
    if (ops_null(ops)) return HSC_EINVAL;
    if (ops->nops > 0x3FFFFFFFull) return HSC_EINVAL;
    if (c->host_only) return HSC_EDEVICE;
    MuGuard g_(c);
    (void)hipSetDevice(c->device);
    hsc_lin_wide_limits lim = {0, 0, 0, 0};
    if (limits) lim = *limits;
    if (!lim.max_configs) lim.max_configs = kLinWideDefaultCap;
    if (!lim.max_expanded) lim.max_expanded = kLinWideDefaultBudget;
    const uint64_t table_bytes = 32ull * lim.max_configs;
    if (lim.max_configs < HSC_LIN_WIDE_MIN_CAP || lim.max_configs > HSC_LIN_WIDE_MAX_CAP ||
        (lim.max_configs & (lim.max_configs - 1)))
        return ctx_fail(c, HSC_EINVAL, "wide linear check: max_configs is not a power of two in range");
    if (lim.flags & ~HSC_LIN_WIDE_ONLY) return ctx_fail(c, HSC_EINVAL, "wide linear check: unknown flags");
    if (!lim.arena_bytes) lim.arena_bytes = kLinWideDefaultArena;
    if (lim.arena_bytes < table_bytes)
        return ctx_fail(c, HSC_EINVAL, "wide linear check: arena_bytes is less than one key's tables");
    if (const char *why = invalid_ops(ops)) return ctx_fail(c, HSC_EINVAL, why);
    const uint32_t nk = ops->nkeys;
    LinearOut &o = c->linear_out;
    reset_out(o, nk);
    memset(out, 0, sizeof *out);
    OpsIndex ix;
    index_ops(ops, ix);
    uint64_t dropped = 0;
    float lds_ms = 0, wide_ms = 0;
    const bool wide_only = (lim.flags & HSC_LIN_WIDE_ONLY) != 0;
    std::vector<uint8_t> pick(std::max<uint32_t>(nk, 1), 0);
    if (!wide_only) {  // exactly hsc_linear_check's pass; what it leaves UNKNOWN goes wide
        Programs p;
        build_programs(ops, ix, nullptr, kLinSlots, 0, o, &dropped, p);
        HIPCHK_RC(c, run_tier(c, p, nullptr, 0, o, &lds_ms, nullptr));
        for (uint32_t k = 0; k < nk; ++k)
            pick[k] = o.verdict[k] == HSC_LIN_UNKNOWN &&
                      (o.cause[k] == HSC_LIN_CAUSE_SLOTS || o.cause[k] == HSC_LIN_CAUSE_CONFIGS);
    } else {  // every key with events (an open read is none)
        for (size_t i = 0; i < ops->nops; ++i)
            if (!(ops->complete[i] == HSC_RT_OPEN && ops->f[i] == HSC_LIN_READ)) pick[ops->key[i]] = 1;
    }
    Programs w;
    build_programs(ops, ix, pick.data(), kLinWideSlots, kLinWideStates, o, wide_only ? &dropped : nullptr, w);
    if (wide_only)  // (the open reads of the keys that have nothing else)
        for (size_t i = 0; i < ops->nops; ++i)
            dropped += !pick[ops->key[i]];
    const LinWideLimits wl = {lim.max_configs, lim.max_expanded};
    const uint32_t per_round = (uint32_t)std::min<uint64_t>(lim.arena_bytes / table_bytes, 0xFFFFFFFFu);
    HIPCHK_RC(c, run_tier(c, w, &wl, per_round, o, &wide_ms, &out->rounds));
    fill_report(o, nk, dropped, lds_ms + wide_ms, &out->base);
    for (uint32_t k = 0; k < nk; ++k) {
        if (!pick[k]) continue;
        o.tier[k] = 1;
        out->escalated++;
        out->resolved += o.verdict[k] != HSC_LIN_UNKNOWN;
        out->wide_expanded += o.expanded[k];
    }
    out->tier = o.tier.data();
    out->table_bytes = table_bytes;
    out->wide_ms = wide_ms;
    return HSC_OK;
}
