"""CPU model of hsc_linear_check_wide (the wide tier): the step
of linear_model.py -- the same event order, lowest-free-slot rule, counts of
sets -- with the slots, the configuration cap, the state limit and the
expansion budget as parameters, and the two-tier report: a key the LDS tier's
caps leave UNKNOWN (slots or configs) is searched again from its first event
at the wide caps and takes every field from that search."""
import math

import numpy as np

import linear_model as LM
from linear_model import BAD, NIL, NONE, OK, UNKNOWN, CAUSE_CONFIGS, CAUSE_SLOTS, _ILLEGAL, apply, key_events

WIDE_SLOTS = 48
WIDE_MIN_CAP, WIDE_MAX_CAP = 8192, 1 << 22
WIDE_STATES = 32767
CAUSE_BUDGET, CAUSE_STATES = 3, 4
DEFAULT_CAP = 1 << 20
DEFAULT_BUDGET = 1 << 25
DEFAULT_ARENA = 1 << 30
NO_BUDGET = math.inf


def check_key(idx, f, a, b, invoke, complete, init=NIL, slots=WIDE_SLOTS, cap=DEFAULT_CAP, max_states=WIDE_STATES,
              budget=DEFAULT_BUDGET):
    """linear_model.check_key with its limits as parameters: ``slots`` ops
    pending at once, ``cap`` configurations alive inside a step, ``max_states``
    distinct non-nil values on the key (None: no limit), and ``budget``: after
    every completed step, more expansions so far than it end the key UNKNOWN /
    BUDGET with peak and final as of the steps done."""
    evs, dropped = key_events(idx, f, invoke, complete)
    out = dict(verdict=OK, cause=0, fail_op=NONE, prev_ok=NONE, peak=1, final=1, possible=[], expanded=0,
               dropped=dropped, events=0)
    used, slot_of = 0, {}
    for _, ret, i in evs:
        if not ret:
            if used == (1 << slots) - 1:
                out.update(verdict=UNKNOWN, cause=CAUSE_SLOTS, peak=0, final=0)
                return out
            s = next(s for s in range(slots) if not used >> s & 1)
            used |= 1 << s
            slot_of[i] = s
        else:
            used &= ~(1 << slot_of[i])
    if max_states is not None and evs:
        vals = {int(init)} | {int(a[i]) for _, ret, i in evs if not ret}
        vals |= {int(b[i]) for _, ret, i in evs if not ret and f[i] == LM.CAS}
        if len(vals - {NIL}) > max_states:
            out.update(verdict=UNKNOWN, cause=CAUSE_STATES, peak=0, final=0)
            return out
    out["events"] = len(evs)
    configs = {(int(init), 0)}
    pend = {}
    prev = NONE
    for _, ret, i in evs:
        s = slot_of[i]
        if not ret:
            pend[s] = (int(f[i]), int(a[i]), int(b[i]))
            continue
        bit = 1 << s
        work = set(configs)
        frontier = [c for c in configs if not c[1] & bit]
        ndone = len(configs) - len(frontier)
        while frontier and len(work) <= cap:
            st, mask = frontier.pop()
            for j, op in pend.items():
                if j == s or mask >> j & 1:
                    continue
                ns = apply(*op, st)
                if ns is not _ILLEGAL and (ns, mask | 1 << j) not in work:
                    work.add((ns, mask | 1 << j))
                    frontier.append((ns, mask | 1 << j))
        if len(work) > cap:
            out.update(verdict=UNKNOWN, cause=CAUSE_CONFIGS, final=len(configs))
            return out
        out["peak"] = max(out["peak"], len(work))
        out["expanded"] += len(work) - ndone
        new = set()
        for st, mask in work:
            if mask & bit:
                new.add((st, mask & ~bit))
            else:
                ns = apply(*pend[s], st)
                if ns is not _ILLEGAL:
                    new.add((ns, mask))
        if not new:
            out.update(verdict=BAD, fail_op=i, prev_ok=prev, final=len(configs),
                       possible=sorted({st for st, _ in configs}))
            return out
        configs = new
        del pend[s]
        prev = i
        out["final"] = len(configs)
        if out["expanded"] > budget:
            out.update(verdict=UNKNOWN, cause=CAUSE_BUDGET)
            return out
    return out


def table_bytes(max_configs):
    """Device bytes of one key's wide tables: two sets of 2 * max_configs words."""
    return 32 * max_configs


def check(ops, init=None, max_configs=None, max_expanded=None, arena_bytes=None, wide_only=False,
          slots=WIDE_SLOTS, max_states=WIDE_STATES):
    """hsc_linear_check_wide's report for ``ops`` as Validator.linear_check_wide
    returns it (less the times): linear_model.check's fields, every key's from
    the tier that judged it, plus ``tier``, ``escalated``, ``resolved``,
    ``rounds``, ``wide_expanded`` and ``table_bytes``.  None: the entry's
    default; ``max_expanded=NO_BUDGET``: no budget."""
    cap = DEFAULT_CAP if max_configs is None else max_configs
    budget = DEFAULT_BUDGET if max_expanded is None else max_expanded
    arena = DEFAULT_ARENA if arena_bytes is None else arena_bytes
    nk = int(ops["nkeys"])
    key = np.asarray(ops["key"])
    cols = [np.asarray(ops[k]) for k in ("f", "a", "b", "invoke", "complete")]
    per, tier = [], np.zeros(nk, np.uint8)
    launched = 0
    for k in range(nk):
        idx = np.flatnonzero(key == k)
        i0 = NIL if init is None else int(init[k])
        p = None if wide_only else LM.check_key(idx, *cols, init=i0)
        if p is None or (p["verdict"] == UNKNOWN and p["cause"] in (CAUSE_SLOTS, CAUSE_CONFIGS)):
            q = check_key(idx, *cols, init=i0, slots=slots, cap=cap, max_states=max_states, budget=budget)
            if p is not None or q["events"] or q["verdict"] == UNKNOWN:  # (WIDE_ONLY: the keys with events)
                tier[k] = 1
                launched += q["events"] > 0
            p = q
        per.append(p)
    wide = [p for k, p in enumerate(per) if tier[k]]
    res = {"nkeys": nk,
           "verdict": np.array([p["verdict"] for p in per], np.uint8),
           "cause": np.array([p["cause"] for p in per], np.uint8),
           "fail_op": np.array([p["fail_op"] for p in per], np.uint32),
           "prev_ok": np.array([p["prev_ok"] for p in per], np.uint32),
           "peak_configs": np.array([p["peak"] for p in per], np.uint32),
           "final_configs": np.array([p["final"] for p in per], np.uint32),
           "possible_values": [[None if v == NIL else v for v in p["possible"]] for p in per],
           "bad": sum(p["verdict"] == BAD for p in per),
           "unknown": sum(p["verdict"] == UNKNOWN for p in per),
           "events": sum(p["events"] for p in per),
           "expanded": sum(p["expanded"] for p in per),
           "dropped_open_reads": sum(p["dropped"] for p in per),
           "tier": tier,
           "escalated": len(wide),
           "resolved": sum(p["verdict"] != UNKNOWN for p in wide),
           "rounds": -(-launched // (arena // table_bytes(cap))),
           "wide_expanded": sum(p["expanded"] for p in wide),
           "table_bytes": table_bytes(cap)}
    return res


# The reference's shape (200 ops at 5 processes, `:info` ops that stay pending)
# past the LDS tier's caps: name -> the generator's arguments.  What the model
# says of them is pinned in test_linear_wide_model.py.
REFERENCE_SHAPES = {
    "valid": dict(seed=2, n_ops=200, n_procs=5, info=0.2, max_open=9),
    "stale": dict(seed=2, n_ops=200, n_procs=5, info=0.2, max_open=10, stale=0.05),
}
REFERENCE_CAP = 1 << 17


def reference_shape(name):
    """The EDN text of REFERENCE_SHAPES[name]."""
    from comdb2_amd import jepsen as J
    return J.cas_register_history_edn(**REFERENCE_SHAPES[name])[0]


WIDE_FIELDS = LM.PARITY_FIELDS + ("tier", "escalated", "resolved", "rounds", "wide_expanded", "table_bytes")


def assert_same(got, want):
    """Device report == model report, field for field."""
    for k in WIDE_FIELDS:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert np.array_equal(np.asarray(g), w), (k, np.asarray(g), w)
        else:
            assert g == w, (k, g, w)
