"""CPU model of hsc_linear_check: knossos.linear's just-in-time
search over configurations (state, pending ops already linearized) as Python
sets, with the entry's event order, slot rule, caps, causes and counts; and the
literal statement of linearizability it is checked against (every choice of
the open ops that happen, every total order that respects real time)."""
import itertools

import numpy as np

READ, WRITE, CAS = 0, 1, 2
NIL = -(1 << 63)
RT_OPEN = 0xFFFFFFFFFFFFFFFF
SLOTS, CAP = 32, 4096
BAD, OK, UNKNOWN = 0, 1, 2
CAUSE_SLOTS, CAUSE_CONFIGS = 1, 2
NONE = 0xFFFFFFFF
_ILLEGAL = object()


def apply(f, a, b, state):
    """The state after op (f, a, b) on ``state`` (NIL: nil), or _ILLEGAL."""
    if f == WRITE:
        return a
    if f == CAS:
        return b if state == a else _ILLEGAL
    return state if a == NIL or a == state else _ILLEGAL


def key_events(idx, f, invoke, complete):
    """(events, dropped open reads) of one key's ops ``idx``: (position, is
    return, op) ordered by position, calls before returns, op index."""
    evs, dropped = [], 0
    for i in idx:
        if complete[i] == RT_OPEN and f[i] == READ:
            dropped += 1
            continue
        evs.append((int(invoke[i]), 0, int(i)))
        if complete[i] != RT_OPEN:
            evs.append((int(complete[i]), 1, int(i)))
    return sorted(evs), dropped


def check_key(idx, f, a, b, invoke, complete, init=NIL):
    """One key's search: dict of verdict, cause, fail_op, prev_ok, peak, final,
    possible (values, NIL first), expanded, dropped, events."""
    evs, dropped = key_events(idx, f, invoke, complete)
    out = dict(verdict=OK, cause=0, fail_op=NONE, prev_ok=NONE, peak=1, final=1, possible=[], expanded=0,
               dropped=dropped, events=0)
    # the lowest free slot at a call, freed at the return
    used, slot_of = 0, {}
    for _, ret, i in evs:
        if not ret:
            if used == (1 << SLOTS) - 1:
                out.update(verdict=UNKNOWN, cause=CAUSE_SLOTS, peak=0, final=0)
                return out
            s = next(s for s in range(SLOTS) if not used >> s & 1)
            used |= 1 << s
            slot_of[i] = s
        else:
            used &= ~(1 << slot_of[i])
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
        while frontier and len(work) <= CAP:
            st, mask = frontier.pop()
            for j, op in pend.items():
                if j == s or mask >> j & 1:
                    continue
                ns = apply(*op, st)
                if ns is not _ILLEGAL and (ns, mask | 1 << j) not in work:
                    work.add((ns, mask | 1 << j))
                    frontier.append((ns, mask | 1 << j))
        if len(work) > CAP:
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
    return out


def check(ops, init=None):
    """hsc_linear_check's report for ``ops`` (the mapping Validator.linear_check
    takes), field for field as that method returns it."""
    nk = int(ops["nkeys"])
    key = np.asarray(ops["key"])
    cols = [np.asarray(ops[k]) for k in ("f", "a", "b", "invoke", "complete")]
    per = [check_key(np.flatnonzero(key == k), *cols, init=NIL if init is None else int(init[k]))
           for k in range(nk)]
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
           "dropped_open_reads": sum(p["dropped"] for p in per)}
    return res


PARITY_FIELDS = ("verdict", "cause", "fail_op", "prev_ok", "peak_configs", "final_configs", "possible_values",
                 "bad", "unknown", "events", "expanded", "dropped_open_reads")


def assert_same(got, want):
    """Device report == model report, field for field."""
    for k in PARITY_FIELDS:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert np.array_equal(np.asarray(g), w), (k, np.asarray(g), w)
        else:
            assert g == w, (k, g, w)


# ---------------------------------------------------------------------------
# the literal statement
# ---------------------------------------------------------------------------
def literal(ops, init=NIL):
    """ops: [(f, a, b, invoke, complete or RT_OPEN)] of one register.  True iff
    for some choice of the open ops that happen there is a total order of the
    closed ops and those, respecting real time (x before y when complete[x] <
    invoke[y]), in which every op is legal."""
    n = len(ops)
    closed = [i for i in range(n) if ops[i][4] != RT_OPEN]
    opened = [i for i in range(n) if ops[i][4] == RT_OPEN]
    before = [[x for x in closed if ops[x][4] < ops[y][3]] for y in range(n)]

    def search(state, left, seen):
        if not left:
            return True
        if (state, left) in seen:
            return False
        seen.add((state, left))
        for y in left:
            if any(x in left for x in before[y]):
                continue
            ns = apply(*ops[y][:3], state)
            if ns is not _ILLEGAL and search(ns, left - {y}, seen):
                return True
        return False

    for r in range(len(opened) + 1):
        for chosen in itertools.combinations(opened, r):
            if search(init, frozenset(closed) | frozenset(chosen), set()):
                return True
    return False


def literal_first_failure(ops, init=NIL):
    """The op at whose completion the literal check first fails on the prefix
    of events up to and including it (ops invoked by then, those not yet
    complete taken as open), or None: the history is linearizable."""
    evs = sorted([(o[3], 0, i) for i, o in enumerate(ops)] +
                 [(o[4], 1, i) for i, o in enumerate(ops) if o[4] != RT_OPEN])
    for e, (_, ret, i) in enumerate(evs):
        if not ret:
            continue
        called = sorted({j for _, r, j in evs[:e + 1] if not r})
        done = {j for _, r, j in evs[:e + 1] if r}
        prefix = [ops[j] if j in done else ops[j][:4] + (RT_OPEN,) for j in called]
        if not literal(prefix, init):
            return i
    return None


def _edn(*ops):
    """Lines from (type, f, value, process) in order; :time = the line."""
    return "".join(f"{{:type :{t} :f :{f} :value {v} :process {p} :time {i + 1}}}\n"
                   for i, (t, f, v, p) in enumerate(ops))


_W1 = (("invoke", "write", 1, 0), ("ok", "write", 1, 0))
_W2 = (("invoke", "write", 2, 0), ("ok", "write", 2, 0))
_W2_OPEN = (("invoke", "write", 2, 1),)
_W2_INFO = (("invoke", "write", 2, 1), ("info", "write", 2, 1))
# the issue's false alarm: w(1) [1,2], w(2) [3,4], w(1) invoked at 5 and completing at 10, read -> 1 over [6,7]
FALSE_ALARM = ("{:type :invoke :f :write :value 1 :process 0 :time 1}\n"
               "{:type :ok :f :write :value 1 :process 0 :time 2}\n"
               "{:type :invoke :f :write :value 2 :process 0 :time 3}\n"
               "{:type :ok :f :write :value 2 :process 0 :time 4}\n"
               "{:type :invoke :f :write :value 1 :process 1 :time 5}\n"
               "{:type :invoke :f :read :value nil :process 2 :time 6}\n"
               "{:type :ok :f :read :value 1 :process 2 :time 7}\n"
               "{:type :ok :f :write :value 1 :process 1 :time 10}\n")
# name -> (EDN, valid, the failing op (invoke order) or None, the values the register could hold before it)
KNOWN = {
    "read_never_written": (_edn(*_W1, ("invoke", "read", "nil", 0), ("ok", "read", 4, 0)), False, 1, [1]),
    "cas_wrong_value_ok": (_edn(*_W1, ("invoke", "cas", "[2 3]", 0), ("ok", "cas", "[2 3]", 0)), False, 1, [1]),
    "nil_read_after_write": (_edn(*_W1, ("invoke", "read", "nil", 0), ("ok", "read", "nil", 0)), True, None, None),
    "stale_read_acked_overwrite": (_edn(*_W1, *_W2, ("invoke", "read", "nil", 0), ("ok", "read", 1, 0)),
                                   False, 2, [2]),
    "stale_read_open_overwrite": (_edn(*_W1, *_W2_OPEN, ("invoke", "read", "nil", 0), ("ok", "read", 1, 0)),
                                  True, None, None),
    "stale_read_info_overwrite": (_edn(*_W1, *_W2_INFO, ("invoke", "read", "nil", 0), ("ok", "read", 1, 0)),
                                  True, None, None),
    "open_write_observed": (_edn(*_W1, *_W2_INFO, ("invoke", "read", "nil", 0), ("ok", "read", 2, 0)),
                            True, None, None),
    "false_alarm": (FALSE_ALARM, True, None, None),
}


def random_ops(rng, n=None):
    """A random one-register history of 2-7 ops over 1-3 values with open ops,
    nil reads, cas and sometimes a non-nil init: ([(f, a, b, invoke, complete)],
    init).  Positions are drawn from a small range, so equal times occur."""
    n = int(rng.integers(2, 8)) if n is None else n
    nv = int(rng.integers(1, 4))
    init = int(rng.integers(1, nv + 1)) if rng.random() < 0.3 else NIL
    ops = []
    for _ in range(n):
        f = int(rng.integers(0, 3))
        a = int(rng.integers(1, nv + 1))
        if f == READ and rng.random() < 0.15:
            a = NIL
        b = int(rng.integers(1, nv + 1)) if f == CAS else NIL
        inv = int(rng.integers(0, 2 * n))
        comp = RT_OPEN if rng.random() < 0.2 else inv + 1 + int(rng.integers(0, n))
        ops.append((f, a, b, inv, comp))
    return ops, init


def one_key(ops):
    """[(f, a, b, invoke, complete)] -> the mapping linear_check takes."""
    f, a, b, inv, comp = (list(c) for c in zip(*ops))
    return columns([dict(f=f, a=a, b=b, invoke=inv, complete=comp)])


def concurrent_writes(k, values=None, read=None, pos0=0):
    """k writes invoked together (write j of values[j], default j + 1), then a
    read (of values[-1] by default) invoked and completed while all are still
    pending, then the writes' completions: the ops as linear_check's columns
    for one key (a dict without nkeys / key)."""
    values = list(range(1, k + 1)) if values is None else list(values)
    f = [WRITE] * k + [READ]
    a = values + [values[-1] if read is None else read]
    invoke = [pos0 + j for j in range(k)] + [pos0 + k]
    complete = [pos0 + k + 2 + j for j in range(k)] + [pos0 + k + 1]
    return dict(f=f, a=a, b=[NIL] * (k + 1), invoke=invoke, complete=complete)


def open_cas(n):
    """n open cas ops, all but [1 2] from values the register never holds (so
    the closure stays small whatever is pending), then a write of 1 and a read
    of it, closed: n + 1 slots in use at once."""
    return dict(f=[CAS] * n + [WRITE, READ], a=[1] + [100 + j for j in range(1, n)] + [1, 1],
                b=[2] * n + [NIL, NIL], invoke=list(range(n)) + [n, n + 2],
                complete=[RT_OPEN] * n + [n + 1, n + 3])


def columns(parts):
    """Per-key column dicts (concurrent_writes' form; None: a key without ops)
    -> the mapping linear_check takes."""
    out = {k: [] for k in ("key", "f", "a", "b", "invoke", "complete")}
    for key, p in enumerate(parts):
        if p is None:
            continue
        out["key"] += [key] * len(p["f"])
        for c in ("f", "a", "b", "invoke", "complete"):
            out[c] += list(p[c])
    res = {"nkeys": len(parts), "key": np.array(out["key"], np.uint32), "f": np.array(out["f"], np.uint8),
           "a": np.array(out["a"], np.int64), "b": np.array(out["b"], np.int64),
           "invoke": np.array(out["invoke"], np.uint64), "complete": np.array(out["complete"], np.uint64)}
    return res
