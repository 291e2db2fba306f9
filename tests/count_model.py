"""Models of the counter and queue checkers.

Two layers.  The plain models restate the reference line for line:
knossos/history.clj's ``complete-fold-op`` with its throws, the loop of
checker/counter (jepsen/checker.clj:240-272), checker/queue's filter and
reduce (:95-101) over jepsen/model.clj's UnorderedQueue and FIFOQueue, and
independent/subhistory (jepsen/independent.clj:239-250).  They are slow and
obviously right.  The numpy formulations restate the passes of hsc_count.hip
-- sorts, scans, gathers -- and return ``Validator.counter_check``'s /
``Validator.queue_check``'s dicts; tests/test_count_model.py holds the two
layers against each other, tests/test_gpu_count.py holds the GPU against the
numpy layer where the plain one would take too long.

Rows are columns as the entries take them: ``type`` 0 invoke, 1 ok, 2 fail, 3
info; counter ``f`` 0 add, 1 read, 2 other; queue ``f`` 0 enqueue, 1 dequeue;
NIL stands for nil.
"""
import collections

import numpy as np

NIL = -(1 << 63)
INVOKE, OK, FAIL, INFO = 0, 1, 2, 3
ADD, READ, OTHER = 0, 1, 2
ENQ, DEQ = 0, 1
V_OK, V_BAD, V_UNKNOWN = 0, 1, 2
NO_ROW = 0xFFFFFFFF
LIST_CAP = 4096


def wrap64(x: int) -> int:
    """x modulo 2^64 as a signed 64-bit value."""
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


# ---------------------------------------------------------------------------
# the plain models
# ---------------------------------------------------------------------------
class Malformed(Exception):
    """What the reference throws; op = the row it throws at."""
    def __init__(self, op: int, kind: int):
        super().__init__(f"op {op} kind {kind}")
        self.op, self.kind = op, kind


def complete(history):
    """history/complete (history.clj:87-171).  history: dicts of ``index``,
    ``type``, ``f``, ``process``, ``value``.  Kinds 1-3 are the reference's
    throws; kind 4 (a completion whose f differs from its invoke's) is this
    project's addition, checked where the reference would go on."""
    out, index = [], {}
    for op in history:
        t, p = op["type"], op["process"]
        if t == INVOKE:
            if p in index:
                raise Malformed(op["index"], 1)
            out.append(dict(op))
            index[p] = len(out) - 1
        elif t == OK:
            if p not in index:
                raise Malformed(op["index"], 2)
            i = index[p]
            if out[i]["f"] != op["f"]:
                raise Malformed(op["index"], 4)
            out[i] = dict(out[i], value=op["value"])
            out.append(dict(op))
            del index[p]
        elif t == FAIL:
            if p not in index:
                raise Malformed(op["index"], 2)
            i = index[p]
            if op["value"] != out[i]["value"]:
                raise Malformed(op["index"], 3)
            if out[i]["f"] != op["f"]:
                raise Malformed(op["index"], 4)
            out[i] = dict(out[i], value=op["value"], fails=True)
            out.append(dict(op))
            del index[p]
        else:
            out.append(dict(op))
    return out


def counter_loop(completed):
    """checker/counter's loop (checker.clj:240-272) over a completed history,
    sums wrapping in 64 bits.  Returns (reads, read ops); a nil where the
    reference's + or <= would throw raises Malformed(kind 5) for the smallest
    such op."""
    lower = upper = 0
    pending, reads, read_ops, nils = {}, [], [], []
    for op in completed:
        tf = (op["type"], op["f"])
        if tf == (INVOKE, READ):
            pending[op["process"]] = (lower, op["value"])
        elif tf == (OK, READ):
            r = pending.pop(op["process"])
            if r[1] == NIL:
                nils.append(op["index"])
            reads.append((r[0], r[1], upper))
            read_ops.append(op["index"])
        elif tf == (INVOKE, ADD):
            if op["value"] == NIL:
                nils.append(op["index"])
            else:
                upper = wrap64(upper + op["value"])
        elif tf == (OK, ADD):
            if op["value"] == NIL:
                nils.append(op["index"])
            else:
                lower = wrap64(lower + op["value"])
    if nils:
        raise Malformed(min(nils), 5)
    return reads, read_ops


def counter_plain(history):
    """One key's report: {"valid": True / False / "unknown", "reads", "errors",
    "read_ops"} or, unknown, {"valid", "op", "kind", "phase"} -- phase
    "complete": where history/complete throws (rows of kind 5 before it are not
    looked at: the comparison with the numpy layer allows for that)."""
    try:
        done = complete(history)
    except Malformed as e:
        return {"valid": "unknown", "op": e.op, "kind": e.kind, "phase": "complete"}
    try:
        reads, ops = counter_loop(done)
    except Malformed as e:
        return {"valid": "unknown", "op": e.op, "kind": e.kind, "phase": "loop"}
    errors = [r for r in reads if not r[0] <= r[1] <= r[2]]
    return {"valid": not errors, "reads": reads, "errors": errors, "read_ops": ops}


class Inconsistent:
    def __init__(self, msg, row, kind):
        self.msg, self.row, self.kind = msg, row, kind


def queue_plain(rows, fifo: bool):
    """(reduce model/step model rows) (checker.clj:95-101): rows = (row index,
    f, value) as the checker's filter leaves them.  Returns {"valid": True,
    "final": ...} -- unordered: sorted (value, multiplicity) pairs; fifo: the
    values in queue order -- or {"valid": False, "row", "kind", "error"}."""
    pending = collections.deque() if fifo else collections.Counter()
    state = None
    for row, f, v in rows:
        if state is not None:  # (Inconsistent absorbs every step)
            continue
        if f == ENQ:
            if fifo:
                pending.append(v)
            else:
                pending[v] += 1
        elif fifo:
            if len(pending) == 0:
                state = Inconsistent(f"can't dequeue {v} from empty queue", row, 2)
            elif v == pending[0]:
                pending.popleft()
            else:
                state = Inconsistent(f"can't dequeue {v}", row, 1)
        else:
            if pending[v] > 0:
                pending[v] -= 1
            else:
                state = Inconsistent(f"can't dequeue {v}", row, 1)
    if state is not None:
        return {"valid": False, "row": state.row, "kind": state.kind, "error": state.msg}
    final = list(pending) if fifo else sorted((v, m) for v, m in pending.items() if m > 0)
    return {"valid": True, "final": final}


def subhistory(k, history):
    """independent/subhistory (independent.clj:239-250): ops whose ``value`` is
    a (key, value) tuple of another key are dropped, those of key k unwrapped,
    every other op kept."""
    out = []
    for op in history:
        v = op["value"]
        if not isinstance(v, tuple):
            out.append(op)
        elif v[0] == k:
            out.append(dict(op, value=v[1]))
    return out


def rows_of_key(cols, key, k):
    """The history dicts of key k from counter columns (type, f, process, value)."""
    t, f, p, v = cols
    return [{"index": i, "type": int(t[i]), "f": int(f[i]), "process": int(p[i]), "value": int(v[i])}
            for i in range(len(t)) if (0 if key is None else int(key[i])) == k]


# ---------------------------------------------------------------------------
# the numpy formulations (the passes of hsc_count.hip)
# ---------------------------------------------------------------------------
def _cols(n, key, nkeys):
    key = np.zeros(n, np.uint32) if key is None else np.asarray(key, np.uint32)
    assert len(key) == n and (n == 0 or int(key.max()) < nkeys)
    return key


def _excl(a):
    """Exclusive wrapping scan, len(a) + 1 entries."""
    out = np.zeros(len(a) + 1, np.uint64)
    np.cumsum(a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64), out=out[1:])
    return out


def counter_np(type_, f, process, value, key=None, nkeys=1):
    """``Validator.counter_check``'s dict (without sort_packed and ms)."""
    t = np.asarray(type_, np.uint8)
    f = np.asarray(f, np.uint8)
    p = np.asarray(process, np.uint32)
    v = np.asarray(value, np.int64)
    n = len(t)
    key = _cols(n, key, nkeys)
    idx = np.arange(n, dtype=np.int64)
    # pair: stable sort by (key, process, is-info), adjacent rows
    order = np.lexsort((idx, t == INFO, p, key))
    st, sf, sv = t[order], f[order], v[order]
    grp = key[order].astype(np.uint64) << np.uint64(32) | p[order]
    same_prev = np.zeros(n, bool)
    same_prev[1:] = grp[1:] == grp[:-1]
    pred_inv = same_prev & (np.roll(st, 1) == INVOKE)
    nxt_ok = np.zeros(n, bool)
    nxt_ok[:-1] = (grp[:-1] == grp[1:]) & (st[1:] == OK)
    is_inv, comp = st == INVOKE, (st == OK) | (st == FAIL)
    eff_s = np.where(is_inv & nxt_ok, np.roll(sv, -1), sv)
    good = comp & pred_inv
    k3 = good & (st == FAIL) & (sv != np.roll(sv, 1))
    k4 = good & ~k3 & (sf != np.roll(sf, 1))
    k5 = good & ~k3 & ~k4 & (st == OK) & (sf != OTHER) & (sv == NIL)
    kind_s = np.zeros(n, np.uint8)
    kind_s[is_inv & pred_inv] = 1
    kind_s[is_inv & ~pred_inv & (sf == ADD) & (eff_s == NIL)] = 5
    kind_s[comp & ~pred_inv] = 2
    kind_s[k3], kind_s[k4], kind_s[k5] = 3, 4, 5
    inv_of = np.full(n, -1, np.int64)
    q = np.flatnonzero(good)
    inv_of[order[q]] = order[q - 1]
    eff = np.empty(n, np.int64)
    eff[order] = eff_s
    malk = np.empty(n, np.uint8)
    malk[order] = kind_s
    none = np.uint64(0xFFFFFFFFFFFFFFFF)
    kmin = np.full(nkeys, none, np.uint64)
    m = malk > 0
    np.minimum.at(kmin, key[m], (idx[m].astype(np.uint64) << np.uint64(3)) | malk[m])
    # key order, scans
    ko = np.argsort(key, kind="stable")
    posof = np.empty(n, np.int64)
    posof[ko] = idx
    khead = np.searchsorted(key[ko], np.arange(nkeys + 1))
    add = f == ADD
    ex_u = _excl(np.where(add & (t == INVOKE), eff, 0)[ko])
    ex_l = _excl(np.where(add & (t == OK), v, 0)[ko])
    # reads
    rp = np.flatnonzero(((t == OK) & (f == READ) & (kmin[key] == none))[ko])
    j = ko[rp]
    h = khead[key[j]]
    lower = (ex_l[posof[inv_of[j]]] - ex_l[h]).view(np.int64)
    upper = (ex_u[rp] - ex_u[h]).view(np.int64)
    val = v[j]
    err = ~((lower <= val) & (val <= upper))
    ex_r = np.zeros(n + 1, np.int64)
    ex_r[rp + 1] = 1
    ex_r = np.cumsum(ex_r)
    read_off = ex_r[khead]
    ex_e = np.concatenate([[0], np.cumsum(err)])
    errors = ex_e[read_off[1:]] - ex_e[read_off[:-1]]
    unknown = kmin != none
    verdict = np.where(unknown, V_UNKNOWN, np.where(errors > 0, V_BAD, V_OK)).astype(np.uint8)
    listed = np.flatnonzero(err)[:LIST_CAP]
    return {"nkeys": nkeys, "bad": int((verdict == V_BAD).sum()), "unknown": int(unknown.sum()),
            "verdict": verdict, "malformed_op": np.where(unknown, kmin >> np.uint64(3), NO_ROW).astype(np.uint32),
            "malformed_kind": np.where(unknown, kmin & np.uint64(7), 0).astype(np.uint8),
            "errors": errors.astype(np.uint32), "read_off": read_off.astype(np.uint32), "reads": len(rp),
            "bad_reads": int(err.sum()), "lower": lower, "value": val, "upper": upper,
            "read_op": j.astype(np.uint32), "n_listed": len(listed), "listed_read": listed.astype(np.uint32)}


def queue_np(f, value, key=None, nkeys=1, fifo=False, final=False):
    """``Validator.queue_check``'s dict (without sort_packed and ms)."""
    f = np.asarray(f, np.uint8)
    v = np.asarray(value, np.int64)
    n = len(f)
    key = _cols(n, key, nkeys)
    idx = np.arange(n, dtype=np.int64)
    big = np.int64(1 << 62)
    emin = np.full(nkeys, big, np.int64)
    if not fifo:
        order = np.lexsort((idx, v, key))
        sk, sv, sf = key[order], v[order], f[order]
        khead = np.searchsorted(sk, np.arange(nkeys + 1))
        head = np.ones(n, bool)
        head[1:] = (sk[1:] != sk[:-1]) | (sv[1:] != sv[:-1])
        rpos = np.concatenate([np.flatnonzero(head), [n]])
        run = np.cumsum(head) - 1
        ex_c = np.concatenate([[0], np.cumsum(np.where(sf == ENQ, 1, -1))])
        cnt = ex_c[1:] - ex_c[rpos[run]] if n else ex_c[1:]
        cand = (sf == DEQ) & (cnt < 0)
        np.minimum.at(emin, sk[cand], order[cand] << 3 | 1)
        bad = emin != big
        flen = np.where(bad, 0, ex_c[khead[1:]] - ex_c[khead[:-1]])
        tot = ex_c[rpos[1:]] - ex_c[rpos[:-1]]
        hp = rpos[:-1]
        keep = (tot > 0) & ~bad[sk[hp]] if n else np.zeros(0, bool)
        fval, fmult = sv[hp[keep]], tot[keep]
        ex_f = np.zeros(n + 1, np.int64)
        ex_f[hp[keep] + 1] = 1
        foff = np.cumsum(ex_f)[khead]
    else:
        ko = np.argsort(key, kind="stable")
        sk, sv, sf = key[ko], v[ko], f[ko]
        khead = np.searchsorted(sk, np.arange(nkeys + 1))
        ex_e = np.concatenate([[0], np.cumsum(sf == ENQ)])
        ex_d = np.concatenate([[0], np.cumsum(sf == DEQ)])
        ev = sv[sf == ENQ]
        dp = np.flatnonzero(sf == DEQ)
        h = khead[sk[dp]]
        kq, b = ex_d[dp] - ex_d[h], ex_e[dp] - ex_e[h]
        empty = b <= kq
        at = np.where(empty, 0, ex_e[h] + kq)
        mism = ~empty & (sv[dp] != (ev[at] if len(ev) else 0))
        kind = np.where(empty, 2, np.where(mism, 1, 0))
        c = kind > 0
        np.minimum.at(emin, sk[dp[c]], ko[dp[c]] << 3 | kind[c])
        bad = emin != big
        ne, nd = ex_e[khead[1:]] - ex_e[khead[:-1]], ex_d[khead[1:]] - ex_d[khead[:-1]]
        flen = np.where(bad, 0, ne - nd)
        foff = np.concatenate([[0], np.cumsum(flen)])
        ep = np.flatnonzero(sf == ENQ)
        r = ex_e[ep] - ex_e[khead[sk[ep]]]
        keep = ~bad[sk[ep]] & (r >= nd[sk[ep]])
        fval, fmult = sv[ep[keep]], np.ones(int(keep.sum()), np.int64)
    if not final:
        fval, fmult, foff = fval[:0], fmult[:0], np.zeros(nkeys + 1, np.int64)
    return {"nkeys": nkeys, "bad": int(bad.sum()), "verdict": np.where(bad, V_BAD, V_OK).astype(np.uint8),
            "error_row": np.where(bad, emin >> 3, NO_ROW).astype(np.uint32),
            "error_kind": np.where(bad, emin & 7, 0).astype(np.uint8), "final_len": flen.astype(np.uint32),
            "final_off": foff.astype(np.uint32), "n_final": len(fval), "final_val": fval.astype(np.int64),
            "final_mult": fmult.astype(np.uint32)}


COUNTER_FIELDS = ("verdict", "malformed_op", "malformed_kind", "errors", "read_off", "lower", "value", "upper",
                  "read_op", "listed_read")
COUNTER_SCALARS = ("nkeys", "bad", "unknown", "reads", "bad_reads", "n_listed")
QUEUE_FIELDS = ("verdict", "error_row", "error_kind", "final_len", "final_off", "final_val", "final_mult")
QUEUE_SCALARS = ("nkeys", "bad", "n_final")


def assert_same(got, want, fields, scalars):
    """Every field of a report against the model's."""
    for k in scalars:
        assert int(got[k]) == int(want[k]), (k, got[k], want[k])
    for k in fields:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if not np.array_equal(a, b):
            i = int(np.flatnonzero(a != b)[0])
            raise AssertionError(f"{k}[{i}]: {a[i]} != {b[i]} ({int((a != b).sum())} differ)")


# ---------------------------------------------------------------------------
# generated columns (vectorised: the GPU tests' and the benchmark's inputs)
# ---------------------------------------------------------------------------
def gen_counter(seed, n_ops, nprocs=4, nkeys=1, proc_mul=1, key_perm=None, fail=0.07, info=0.08, differ=0.05,
                lo_add=1, hi_add=6):
    """A well-formed counter history of n_ops ops (two rows each, an :info op's
    process retires) as (type, f, process, value, key): batches of nprocs
    concurrent ops, half adds of [lo_add, hi_add) and half reads; ``differ`` of
    the ok adds complete with another value than they invoked.  Read values
    are placeholders: :func:`set_reads` places them against the bounds.
    ``proc_mul``: process ids are multiplied by it (wide ids for the unpacked
    sort path)."""
    rng = np.random.default_rng(seed)
    nb = -(-n_ops // nprocs)
    m = nb * nprocs
    comp = rng.choice(np.array([OK, FAIL, INFO], np.uint8), m, p=[1 - fail - info, fail, info]).reshape(nb, nprocs)
    retired = np.cumsum(comp == INFO, axis=0) - (comp == INFO)
    proc = (np.arange(nprocs)[None, :] + nprocs * retired).astype(np.uint64) * np.uint64(proc_mul)
    f = rng.integers(0, 2, m).astype(np.uint8)
    val = rng.integers(lo_add, hi_add, m).astype(np.int64)
    cval = np.where((rng.random(m) < differ) & (comp.ravel() == OK), rng.integers(lo_add, hi_add, m), val)
    key = rng.integers(0, nkeys, m).astype(np.uint32)
    t_inv = np.arange(m) // nprocs + rng.random(m) * 0.5
    t_cmp = t_inv + 0.01 + rng.random(m) * 0.45
    order = np.argsort(np.concatenate([t_inv, t_cmp]), kind="stable")
    is_c = order >= m
    op = np.where(is_c, order - m, order)
    keep = op < n_ops
    is_c, op = is_c[keep], op[keep]
    type_ = np.where(is_c, comp.ravel()[op], INVOKE).astype(np.uint8)
    value = np.where(is_c, cval[op], val[op])
    value = np.where((f[op] == READ) & (~is_c | (type_ == FAIL)), NIL, value)  # (a failed read keeps its nil)
    k = key[op] if key_perm is None else np.asarray(key_perm, np.uint32)[key[op]]
    return type_, f[op], (proc.ravel()[op] & np.uint64(0xFFFFFFFF)).astype(np.uint32), value.astype(np.int64), k


def set_reads(cols, nkeys, mode="mixed"):
    """Place the ok reads' values against their bounds (which no read value
    moves): mode "mixed" cycles lower - 1, lower, upper, upper + 1 and a value
    inside; "good" takes lower; "bad" upper + 1."""
    t, f, p, v, key = cols
    m = counter_np(t, f, p, v, key, nkeys)
    v = v.copy()
    lo, hi = m["lower"], m["upper"]
    c = np.arange(len(lo)) % 5
    pick = {"mixed": np.select([c == 0, c == 1, c == 2, c == 3], [lo - 1, lo, hi, hi + 1], lo + (hi - lo) // 2),
            "good": lo, "bad": hi + 1}[mode]
    v[m["read_op"]] = pick
    return t, f, p, v, key


def gen_queue(seed, n, nkeys=1, p_enq=0.6, nvalues=40, mismatch=0.0, value_mul=1, key_perm=None):
    """Queue rows (f, value, key): a dequeue takes the value of its key's
    enqueue of the same rank (fifo-legal whenever that enqueue came first; an
    "empty" error otherwise), ``mismatch`` of them another value."""
    rng = np.random.default_rng(seed)
    f = (rng.random(n) >= p_enq).astype(np.uint8)
    key = rng.integers(0, nkeys, n).astype(np.uint32)
    v = rng.integers(0, nvalues, n).astype(np.int64) * value_mul
    ko = np.argsort(key, kind="stable")
    sk, sf = key[ko], f[ko]
    khead = np.searchsorted(sk, np.arange(nkeys + 1))
    ex_e = np.concatenate([[0], np.cumsum(sf == ENQ)])
    ex_d = np.concatenate([[0], np.cumsum(sf == DEQ)])
    ev = v[ko][sf == ENQ]
    dp = np.flatnonzero(sf == DEQ)
    at = ex_e[khead[sk[dp]]] + ex_d[dp] - ex_d[khead[sk[dp]]]
    has = at < ex_e[khead[sk[dp] + 1]]
    src = np.where(has, at, 0)
    if len(ev):
        take = has & (rng.random(len(dp)) >= mismatch)
        v[ko[dp[take]]] = ev[src[take]]
    if key_perm is not None:
        key = np.asarray(key_perm, np.uint32)[key]
    return f, v, key
