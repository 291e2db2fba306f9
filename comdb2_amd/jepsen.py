"""Jepsen-format histories -> dependency-graph histories.

The reference's Jepsen harness records operation histories as EDN, one map
per line, an ``:invoke`` and its completion (``:ok`` / ``:fail`` / ``:info``)
per process:

* the C register client (linearizable/ctest/register.c:282-370): one
  register (``id = 1``), ``:f :read`` (completes with the observed ``:value``
  and ``:uid``, ``nil`` for an empty register), ``:f :write :value v :uid u``
  and ``:f :cas :value [cur new] :uid u`` (``update ... where val = cur``);
  every txn runs SERIALIZABLE (register.c:270);
* Adya's G2 workload (linearizable/jepsen/src/jepsen/adya.clj:13-55):
  ``:f :insert :value [key [a-id b-id]]`` -- the txn reads tables a and b for
  the key and inserts its row into one of them only if both were empty; the
  G2 checker (:57-83) flags a key with more than one ``:ok`` insert.

:func:`history_from_jepsen_edn` pairs each invoke with its completion (a
history may also be one EDN vector of ops, as knossos reads it:
linearizable/filetest/src/jepsen/filetest.clj, ``history.txt``), drops
``:fail`` ops (not committed), and turns every ``:ok`` op into one committed
transaction of a :class:`workloads.History`:

* txn ids = commit order, taken as the order of the completions (their
  ``:time``, else their line order); a key's version order is its writers'
  txn order;
* register read: a read of the version it returned -- the writer with the
  same ``:uid`` and value when the op carries a ``:uid`` (register.c), else
  the writer of the same value (a knossos register history of unique
  values); the latest such writer before it, else the earliest after it;
  ``nil`` = the initial, empty register;
* register write: a write of the register;
* register cas ``[cur new]``: a read of the latest earlier version whose value
  is ``cur`` (the version the ``where val = cur`` matched: the CAS chain)
  plus a write;
* insert ``[k [a b]]``: reads of ``(k, a)`` and ``(k, b)`` that saw the
  initial (absent) rows, plus a write of ``(k, a)`` or ``(k, b)``.

``:info`` ops are indeterminate: they may have committed.  Their writes stay
candidate versions, and one that a read observed (no ``:ok`` writer produced
that version) did commit -- it joins the history as a transaction ordered at
its invoke (``info_recovered``); the others are dropped.  Reads whose version
no writer produced are dropped and counted (``dangling``).  hsc_dep_graph_*
then builds the WR / WW / RW edges and the SCCs; a nontrivial SCC is a
dependency cycle (two ``:ok`` inserts of one G2 key form the 2-cycle of rw
edges the G2 checker looks for).

``check_edn(..., isolation=True)`` also answers whether a history that is not
serializable is at least snapshot isolation (comdb2 ships that level as
``enable_snapshot_isolation``; adya.clj's write skew is legal under it).  That
verdict is the dependency-graph condition only -- every cycle has two adjacent
anti-dependency edges -- over the committed txns: the register / insert
conversion above drops ``:fail`` ops and resolves reads to writer txns, so
``check_edn`` does not model aborted and intermediate reads (G1a, G1b).

The value entry does.  :func:`vhistory_from_txn_edn` reads multi-op txn
histories (``:f :txn :value [[:r k v] [:w k v] ...]``, Elle's rw-register
form) into a :class:`workloads.ValueHistory` of every attempted txn -- ``:ok``,
``:fail`` (aborted) and ``:info`` / unpaired (unknown) alike -- and
:func:`check_txn_edn` has the GPU find the write each read observed
(``Validator.dep_graph_resolve``), report G1a / G1b, decide which unknown txns
committed, and run the analyses of ``check_edn`` on the committed part.
:func:`check_dirty_reads_edn` does the resolve alone for the reference's
dirty-reads workload (linearizable/jepsen/src/comdb2/core.clj:320-353,
:492-523: "a failed transaction whose value became visible to some read").
Internal consistency (a txn reading its own earlier ops, Elle's ``:internal``)
is checked on request: ``check_txn_edn(..., internal=True)`` and
``check_append_edn(..., internal=True)`` run ``Validator.graph_internal`` /
``graph_internal_lists`` on the history the resolve uploaded
(:func:`internal_reads`, :func:`internal_list_reads`, :func:`with_internal`).

Both conversions above take completion order for commit order, which a Jepsen
history does not carry.  A list-append history needs no such premise:
:func:`lhistory_from_append_edn` reads Elle's ``[:append k v]`` / ``[:r k [v
...]]`` form into a :class:`workloads.ListHistory`, and
:func:`check_append_edn` has the GPU recover every key's version order from
its longest read (``Validator.graph_resolve_lists``), report G1a / G1b,
incompatible orders and duplicated elements, and run the same analyses on the
edges that order gives.

A register history without ``:uid`` (the reference's Clojure register
workload: ``rand-int 5`` values) gives value matching nothing to tell two
writers of one value apart, so the register conversion above is a guess there.
:func:`check_linear_edn` judges such a history the way the reference does, by
knossos' linearizability search over the cas-register model
(``Validator.linear_check``: a search per key on the GPU, no graph), and
:func:`cas_register_history_edn` generates histories of that form.

The suite's other two workloads are neither graphs nor searches but
accounting, and their checkers filter ops by ``:type`` and ``:f`` without
pairing invokes and completions; so do the conversions here.
:func:`check_set_edn` is ``checker/set`` (jepsen/checker.clj:108-154: attempted
adds, acknowledged adds and the final read compared as sets; a set ``#{...}``
parses as a list), :func:`check_total_queue_edn` is ``checker/total-queue``
(:163-218, the same over multisets) -- both one ``Validator.tally_check`` -- and
:func:`check_bank_edn` is the bank test's ``bank-checker`` (core.clj:152-177:
every read's length and total against the model, ``Validator.bank_check``).
:func:`set_report`, :func:`total_queue_report` and :func:`bank_report` are the
pure halves; :func:`set_history_edn`, :func:`queue_history_edn` and
:func:`bank_history_edn` generate histories with known injections.

Every composed checker of core.clj also carries ``:perf (checker/perf)``
(jepsen/checker.clj:288-309, jepsen/checker/perf.clj): the data sets of the
latency, latency-quantile and rate graphs.  :func:`check_perf_edn` produces
them (``Validator.perf_check``; :func:`perf_ops_from_edn` interns the history,
:func:`perf_report` is the pure half), :func:`with_times` stamps ``:time`` on
a generated history, and :func:`compose_edn` is ``checker/compose`` with
``merge-valid`` (:func:`merge_valid`; checker.clj:20-35, :274-286) over the
checkers of this module.
"""
from __future__ import annotations

import collections
import dataclasses
import decimal
import fractions
import re
from typing import Dict, List, Optional, Tuple

import numpy as np

from .workloads import TXN_ABORTED, TXN_OK, TXN_UNKNOWN, VAL_INIT, History, ListHistory, ValueHistory

# ---------------------------------------------------------------------------
# EDN (the subset the histories use: maps, vectors, keywords, integers, nil,
# booleans, strings)
# ---------------------------------------------------------------------------
_TOK = re.compile(r'\s*(?:,\s*)*([{}\[\]()]|"(?:[^"\\]|\\.)*"|[^\s,{}\[\]()"]+)')


def _tokens(text: str):
    pos = 0
    while True:
        m = _TOK.match(text, pos)
        if not m or m.end() == pos:
            return
        pos = m.end()
        yield m.group(1)


def _parse(tokens, tok):
    if tok == "#":  # a set #{...} (the set workload's final read): its elements as a list
        if next(tokens, None) != "{":
            raise ValueError("unsupported EDN dispatch form")
        tok = "#{"
    if tok in ("{", "[", "(", "#{"):
        close = {"{": "}", "[": "]", "(": ")", "#{": "}"}[tok]
        items = []
        for t in tokens:
            if t == close:
                break
            items.append(_parse(tokens, t))
        else:
            raise ValueError("unterminated EDN collection")
        if tok == "{":
            if len(items) % 2:
                raise ValueError("odd EDN map")
            return dict(zip(items[::2], items[1::2]))
        return items
    if tok in ("}", "]", ")"):
        raise ValueError(f"unexpected {tok!r}")
    if tok == "nil":
        return None
    if tok in ("true", "false"):
        return tok == "true"
    if tok.startswith('"'):
        return tok[1:-1]
    if re.fullmatch(r"[-+]?\d+N?", tok):
        return int(tok.rstrip("N"))
    return tok  # keywords stay strings (":ok")


def parse_edn(text: str) -> List:
    """Every top-level EDN form of text, in order."""
    toks = _tokens(text)
    return [_parse(toks, t) for t in toks]


# ---------------------------------------------------------------------------
# history -> dependency-graph ops
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class JepsenOps:
    """What the conversion kept and dropped."""
    history: History
    ok: int                  # completed :ok ops (committed txns)
    failed: int              # :fail completions (dropped)
    info: int                # :info completions (indeterminate)
    unpaired: int            # invokes without a completion
    dangling: int            # reads of a version no writer produced (dropped)
    g2_keys: Dict[int, int]  # insert key -> :ok inserts (adya.clj g2-checker input)
    txn_ops: List[dict]      # the completion of each txn (txn id order)
    info_recovered: int = 0  # :info ops whose write a read observed (committed)
    # each txn's interval in real time (txn id order): an :ok op's is [its
    # invoke, its completion], a recovered :info op's [its invoke, RT_OPEN]
    # (it never completed); a completion without an invoke starts at itself.
    # ``:time`` when every paired op carries an integer one, else line indices
    # for all ops alike.
    invoke: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint64))
    complete: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint64))


def _flatten(forms):
    for f in forms:
        if isinstance(f, list):  # a history vector [op op ...]
            yield from _flatten(f)
        else:
            yield f


def _pairs(forms):
    """(ok, info, failed, unpaired): ok / info = [(invoke, completion, line,
    the invoke's line or -1)]."""
    pending: Dict[object, Tuple[dict, int]] = {}
    done, infos, failed = [], [], 0
    for i, op in enumerate(_flatten(forms)):
        if not isinstance(op, dict):
            continue
        t, p = op.get(":type"), op.get(":process")
        if t == ":invoke":
            pending[p] = (op, i)
        elif t in (":ok", ":fail", ":info"):
            inv, il = pending.pop(p, (None, -1))
            if t == ":fail":
                failed += 1
            elif t == ":info":
                infos.append((inv or {}, op, i, il))
            else:
                done.append((inv or {}, op, i, il))
    return done, infos, failed, len(pending)


_INSERT_TABLES = 2  # adya.clj: tables a and b


def _time(op, line):
    t = op.get(":time")
    return t if isinstance(t, int) else line


def history_from_jepsen_edn(text: str) -> JepsenOps:
    """See the module docstring.  Register keys are ``:key`` when an op
    carries one (the reference's client has a single register, id 1); G2
    insert keys become (key, table) = 2 key + {0: a, 1: b}."""
    done, infos, failed, unpaired = _pairs(parse_edn(text))
    # every op that may be a txn: (order time, line, invoke, completion, is :ok)
    # -- an :ok op commits at its completion, an :info op (if at all) by its
    # completion, taken as its invoke
    cands = [(_time(op, i), i, inv, op, True) for inv, op, i, _ in done]
    cands += [(_time(inv, i) if inv else i, i, inv, op, False) for inv, op, i, _ in infos
              if op.get(":f", inv.get(":f")) in (":write", ":cas")]
    cands.sort(key=lambda c: (c[0], c[1]))
    # per candidate: its ops as (key, is_write, read kind, a, b)
    ops_of: List[List[tuple]] = []
    writers: Dict[int, List[Tuple[int, object, object]]] = {}  # key -> [(cand, uid, value)]
    g2: Dict[int, int] = {}
    for c, (_, _, inv, op, ok) in enumerate(cands):
        f = op.get(":f", inv.get(":f"))
        mine = []
        if f in (":read", ":write", ":cas"):
            k = int(op.get(":key", inv.get(":key", 1)))
            if f == ":read":
                if ":uid" in op:
                    mine.append((k, 0, "uid", op.get(":uid"), op.get(":value")))
                else:
                    mine.append((k, 0, "value", op.get(":value"), None))
            else:
                val = op.get(":value", inv.get(":value"))
                if f == ":cas":
                    cur, val = val
                    mine.append((k, 0, "cas", cur, None))
                writers.setdefault(k, []).append((c, op.get(":uid", inv.get(":uid")), val))
                mine.append((k, 1, None, None, None))
        elif f == ":insert":
            k, (a_id, b_id) = op.get(":value", inv.get(":value"))
            g2[int(k)] = g2.get(int(k), 0) + 1
            for tb in range(_INSERT_TABLES):  # both tables read empty
                mine.append((2 * int(k) + tb, 0, "none", None, None))
            mine.append((2 * int(k) + (0 if a_id is not None else 1), 1, None, None, None))
        ops_of.append(mine)

    def observed(c, k, kind, a, b):
        """The candidate whose version a read of candidate c saw (None:
        initial; -1: no writer produced it)."""
        if kind == "none" or (kind in ("uid", "value") and a is None):
            return None
        ws = writers.get(k, [])
        if kind == "cas":
            hits = [w for w, u, v in reversed(ws) if w < c and v == a]
            hits = [w for w in hits if cands[w][4]] or hits  # :ok writers first
            return hits[0] if hits else -1
        if kind == "uid":
            match = [w for w, u, v in ws if u == a and (b is None or v == b)]
        else:
            match = [w for w, u, v in ws if v == a]
        for pool in ([w for w in match if cands[w][4]], match):  # :ok writers first
            before = [w for w in pool if w < c]
            if before:
                return before[-1]
            if pool:
                return pool[0]
        return -1

    keep = [c[4] for c in cands]  # :ok ops; observed :info writes join below
    seen: Dict[Tuple[int, int], object] = {}
    for c, mine in enumerate(ops_of):
        if not cands[c][4]:
            continue
        for j, (k, w, kind, a, b) in enumerate(mine):
            if not w:
                seen[(c, j)] = observed(c, k, kind, a, b)
    # an :info write a committed read observed did commit (and its own reads
    # then count too)
    changed = True
    while changed:
        changed = False
        for (c, j), hit in list(seen.items()):
            if isinstance(hit, int) and hit >= 0 and not keep[hit]:
                keep[hit] = True
                changed = True
                for jj, (k, w, kind, a, b) in enumerate(ops_of[hit]):
                    if not w:
                        seen[(hit, jj)] = observed(hit, k, kind, a, b)
    tid = {}
    for c in range(len(cands)):
        if keep[c]:
            tid[c] = len(tid)
    txn, key, isw, obs = [], [], [], []
    dangling = 0
    for c, mine in enumerate(ops_of):
        if not keep[c]:
            continue
        for j, (k, w, kind, a, b) in enumerate(mine):
            o = -1
            if not w:
                hit = seen.get((c, j))
                if hit is not None and (hit < 0 or not keep[hit]):
                    dangling += 1
                    continue
                o = -1 if hit is None else tid[hit]
            txn.append(tid[c]), key.append(k), isw.append(w), obs.append(o)
    h = History(np.array(txn, np.uint32), np.array(key, np.uint64), np.array(isw, np.uint8),
                np.array(obs, np.int64), len(tid))
    recovered = sum(1 for c in range(len(cands)) if keep[c] and not cands[c][4])
    invoke, complete = _intervals(done, infos, [cands[c] for c in range(len(cands)) if keep[c]])
    return JepsenOps(h, len(done), failed, len(infos), unpaired, dangling, g2,
                     [cands[c][3] for c in range(len(cands)) if keep[c]], recovered, invoke, complete)


RT_OPEN = 0xFFFFFFFFFFFFFFFF  # HSC_RT_OPEN: the txn never completed


def _intervals(done, infos, kept):
    """(invoke, complete) of the kept candidates (JepsenOps.invoke / .complete)."""
    paired = [o for inv, op, _, il in done + infos for o in ((inv, op) if il >= 0 else (op,))]
    use_time = all(type(o.get(":time")) is int for o in paired)
    inv_line = {i: il for _, _, i, il in done + infos}  # by the completion's line
    rows = []
    for _, i, inv, op, ok in kept:
        il = inv_line[i]
        end = op[":time"] if use_time else i
        start = end if il < 0 else (inv[":time"] if use_time else il)
        rows.append((min(start, end), end if ok else None))
    base = min([0] + [r[0] for r in rows])  # (a clock that starts below zero)
    invoke = np.array([a - base for a, _ in rows], np.uint64)
    complete = np.array([RT_OPEN if b is None else b - base for _, b in rows], np.uint64)
    return invoke, complete


def g2_illegal(ops: JepsenOps) -> Dict[int, int]:
    """adya.clj g2-checker (:57-83): the insert keys with more than one :ok
    insert."""
    return {k: c for k, c in ops.g2_keys.items() if c > 1}


# ---------------------------------------------------------------------------
# which anomaly, and the transactions to look at
# ---------------------------------------------------------------------------
ANOMALY_NAMES = {1: "G1c", 2: "G-single", 4: "G2"}  # hsc_anomalies class bits
_EDGE_BITS = ((1, "ww"), (2, "wr"), (4, "rw"), (8, "rt"))


def edge_type_name(bits: int) -> str:
    """"ww" / "wr" / "rw" / "rt" (the real-time order); an edge merged from
    several dependencies joins their names with "+" ("wr+rw", "rw+rt")."""
    return "+".join(n for b, n in _EDGE_BITS if bits & b)


def anomaly_report(ops: JepsenOps, result: dict) -> dict:
    """What a reader of a Jepsen result asks of
    ``Validator.dep_graph_anomalies()``'s dict (a pure function of its
    arguments): ``valid`` -- no dependency cycle; ``anomaly_types`` -- the
    sorted classes of the components ("G1c" circular information flow,
    "G-single" read skew, "G2" an anti-dependency cycle); ``cycles`` -- one
    entry per component: its ``type``, ``label`` (the component's largest
    txn), and from the witness its ``txns`` in cycle order, ``edge_types``
    (the dependency of each step txns[i] -> txns[i + 1], the last one back to
    txns[0]) and ``ops`` (the txns' completions, ``ops.txn_ops``) -- empty
    lists when the analysis ran without witnesses; ``g2_keys`` -- adya.clj's
    own verdict (:func:`g2_illegal`)."""
    labels = [int(x) for x in result.get("comp_label", ())]
    classes = [int(x) for x in result.get("comp_class", ())]
    off = [int(x) for x in result.get("wit_off", ())]
    wt = [int(x) for x in result.get("wit_txn", ())]
    wy = [int(x) for x in result.get("wit_type", ())]
    if len(off) != len(labels) + 1:
        off = [0] * (len(labels) + 1)
    cycles = []
    for i, (lab, k) in enumerate(zip(labels, classes)):
        txns = wt[off[i]:off[i + 1]]
        cycles.append({"type": ANOMALY_NAMES[k], "label": lab, "txns": txns,
                       "edge_types": [edge_type_name(t) for t in wy[off[i]:off[i + 1]]],
                       "ops": [ops.txn_ops[t] for t in txns]})
    return {"valid": not labels, "anomaly_types": sorted({c["type"] for c in cycles}),
            "cycles": cycles, "g2_keys": g2_illegal(ops)}


def isolation_report(ops: JepsenOps, result: dict, si: dict, strict: Optional[dict] = None,
                     strict_si: Optional[dict] = None) -> dict:
    """The snapshot-isolation part of a report (a pure function of its
    arguments): ``result`` is ``Validator.dep_graph_anomalies()``'s dict and
    ``si`` ``Validator.dep_graph_si()``'s, both of the plain build; ``strict``
    / ``strict_si`` the same two of the build with the real-time order, when
    there was one.  ``snapshot_isolation_valid`` -- no component holds a cycle
    without two adjacent anti-dependency edges; ``si_cycles`` -- one entry per
    flagged component, shaped as :func:`anomaly_report`'s ``cycles`` and built
    from the SI witness, ``type`` "G-nonadjacent" when the component's plain
    class is G2 (two or more anti edges, none adjacent), else the plain class
    name; ``levels`` -- ``g1c_free`` (no txn on a cycle of ww / wr edges),
    ``snapshot_isolation``, ``serializable``, with ``strict``
    ``strict_serializable`` and with ``strict_si`` too
    ``strong_snapshot_isolation``.  All of it is the dependency-graph
    condition over committed txns: G1a / G1b are :func:`check_txn_edn`'s
    (``levels["read_committed"]``), not this function's."""
    labels = [int(x) for x in si.get("comp_label", ())]
    flagged = [int(x) for x in si.get("comp_nonadj", ())]
    plain = {int(l): int(k) for l, k in zip(result.get("comp_label", ()), result.get("comp_class", ()))}
    off = [int(x) for x in si.get("wit_off", ())]
    wt = [int(x) for x in si.get("wit_txn", ())]
    wy = [int(x) for x in si.get("wit_type", ())]
    if len(off) != len(labels) + 1:
        off = [0] * (len(labels) + 1)
    cycles = []
    for i, (lab, f) in enumerate(zip(labels, flagged)):
        if not f:
            continue
        k = plain[lab]
        txns = wt[off[i]:off[i + 1]]
        cycles.append({"type": "G-nonadjacent" if k == 4 else ANOMALY_NAMES[k], "label": lab, "txns": txns,
                       "edge_types": [edge_type_name(t) for t in wy[off[i]:off[i + 1]]],
                       "ops": [ops.txn_ops[t] for t in txns]})
    levels = {"g1c_free": int(result["txns"][0]) == 0, "snapshot_isolation": not any(flagged),
              "serializable": len(result.get("comp_label", ())) == 0}
    if strict is not None:
        levels["strict_serializable"] = len(strict.get("comp_label", ())) == 0
        if strict_si is not None:
            levels["strong_snapshot_isolation"] = not any(int(x) for x in strict_si.get("comp_nonadj", ()))
    return {"snapshot_isolation_valid": not any(flagged), "si_cycles": cycles, "levels": levels}


def check_edn(validator, text: str, witness: bool = True, realtime: bool = False,
              isolation: bool = False) -> dict:
    """A Jepsen EDN history through the GPU: convert, build the typed graph,
    classify its cycles; :func:`anomaly_report`'s dict plus ``history`` (the
    :class:`JepsenOps`) and ``analysis`` (dep_graph_anomalies' dict).

    ``realtime``: also the strict-serializability (linearizability of whole
    txns) verdict.  After the plain pass the real-time order of the txns'
    intervals (``JepsenOps.invoke`` / ``.complete``) is staged as "rt" edges,
    the graph built and analysed again, and the report gains ``strict_valid``
    (the second build has no component of >= 2 txns); ``realtime_cycles`` --
    one entry shaped as those of ``cycles`` per component of the second build
    none of whose txns has a nonzero ``cls`` in the plain pass, the anomalies
    that exist only because of real time (each of their cycles takes an rt
    edge), ``type`` = the class name + "-realtime"; ``realtime_anomaly_types``
    (their sorted types); ``realtime_analysis`` -- the second analysis dict
    plus ``edges`` (rt edges staged) and ``stage_ms`` (their device time).
    ``valid``, ``anomaly_types`` and ``cycles`` keep describing the plain
    pass.

    ``isolation``: also the snapshot-isolation verdict of the plain pass
    (``Validator.dep_graph_si``): the report gains :func:`isolation_report`'s
    ``snapshot_isolation_valid``, ``si_cycles`` and ``levels``, and
    ``si_analysis`` (dep_graph_si's dict).  With ``realtime`` as well the
    analysis runs again on the real-time build and ``levels`` has
    ``strong_snapshot_isolation``.  Aborted and intermediate
    reads are not modelled by this conversion (the module docstring;
    :func:`check_txn_edn` models them)."""
    ops = history_from_jepsen_edn(text)
    return _check_built(validator, ops, lambda: validator.dep_graph_build(ops.history, full=True),
                        ops.history.ntxn, witness, realtime, isolation)


def _check_built(validator, ops, build, ntxn: int, witness: bool, realtime: bool, isolation: bool) -> dict:
    """check_edn from the build on: ``build()`` builds the full graph of the
    ntxn txns whose completions and intervals ``ops`` holds."""
    build()
    result = validator.dep_graph_anomalies(witness=witness)
    report = anomaly_report(ops, result)
    report["history"] = ops
    report["analysis"] = result
    si = validator.dep_graph_si(witness=witness) if isolation else None
    if not realtime:
        if isolation:
            report.update(isolation_report(ops, result, si))
            report["si_analysis"] = si
        return report
    staged = validator.dep_graph_stage_realtime(ops.invoke, ops.complete)
    build()
    strict = dict(validator.dep_graph_anomalies(witness=witness))
    scc, _ = validator.dep_graph_scc_built(ntxn)
    strict["edges"], strict["stage_ms"] = staged["edges"], staged["ms"]
    plain_cls = np.asarray(result["cls"])
    cycles = []
    for c, lab in zip(anomaly_report(ops, strict)["cycles"], strict["comp_label"]):
        if not plain_cls[np.asarray(scc) == lab].any():
            cycles.append(dict(c, type=c["type"] + "-realtime"))
    report["strict_valid"] = len(strict["comp_label"]) == 0
    report["realtime_cycles"] = cycles
    report["realtime_anomaly_types"] = sorted({c["type"] for c in cycles})
    report["realtime_analysis"] = strict
    if isolation:
        strict_si = validator.dep_graph_si(witness=witness)
        report.update(isolation_report(ops, result, si, strict, strict_si))
        report["si_analysis"] = si
    return report


# ---------------------------------------------------------------------------
# value histories: every attempted txn, reads resolved on the GPU
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class TxnOps:
    """Every attempted txn of a history, in txn id order."""
    vhistory: ValueHistory
    ok: int                  # :ok completions (TXN_OK)
    failed: int              # :fail completions (TXN_ABORTED)
    info: int                # :info completions (TXN_UNKNOWN)
    unpaired: int            # invokes without a completion (TXN_UNKNOWN)
    txn_ops: List[dict]      # the completion of each txn (an unpaired txn's invoke)
    # each txn's interval (JepsenOps.invoke / .complete): an :ok or :fail op's
    # is [its invoke, its completion], any other's [its invoke, RT_OPEN]
    invoke: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint64))
    complete: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint64))
    g2_keys: Dict[int, int] = dataclasses.field(default_factory=dict)  # (anomaly_report reads it: none here)


def _attempts(text: str, fs) -> List[tuple]:
    """Every op whose :f is in fs as an attempted txn, in txn id order:
    (invoke or {}, completion or None, status, line of the invoke or -1, line
    of the completion or -1).  Ids run in order of (completion time for :ok /
    :fail, invoke time for the others, then line), as history_from_jepsen_edn
    orders its candidates."""
    pending: Dict[object, Tuple[dict, int]] = {}
    rows = []
    for i, op in enumerate(_flatten(parse_edn(text))):
        if not isinstance(op, dict):
            continue
        t, p = op.get(":type"), op.get(":process")
        if t == ":invoke":
            pending[p] = (op, i)
        elif t in (":ok", ":fail", ":info"):
            inv, il = pending.pop(p, (None, -1))
            if op.get(":f", (inv or {}).get(":f")) not in fs:
                continue
            if t == ":info":
                rows.append((_time(inv, il) if inv else i, il if inv else i, inv or {}, op, TXN_UNKNOWN, il, i))
            else:
                rows.append((_time(op, i), i, inv or {}, op, TXN_OK if t == ":ok" else TXN_ABORTED, il, i))
    for inv, il in pending.values():
        if inv.get(":f") in fs:
            rows.append((_time(inv, il), il, inv, None, TXN_UNKNOWN, il, -1))
    rows.sort(key=lambda r: (r[0], r[1]))
    return [r[2:] for r in rows]


def _attempt_intervals(att) -> Tuple[np.ndarray, np.ndarray]:
    seen = [o for inv, op, _, il, cl in att for o in ((inv,) if il >= 0 else ()) + ((op,) if op is not None else ())]
    use_time = all(type(o.get(":time")) is int for o in seen)
    rows = []
    for inv, op, st, il, cl in att:
        end = None if op is None else (op[":time"] if use_time else cl)
        start = end if il < 0 else (inv[":time"] if use_time else il)
        rows.append((start if end is None else min(start, end), end if st != TXN_UNKNOWN else None))
    base = min([0] + [r[0] for r in rows])
    return (np.array([a - base for a, _ in rows], np.uint64),
            np.array([RT_OPEN if b is None else b - base for _, b in rows], np.uint64))


def _txn_ops_record(att, txn, key, isw, val) -> TxnOps:
    status = np.array([a[2] for a in att], np.uint8)
    vh = ValueHistory(np.array(txn, np.uint32), np.array(key, np.uint64), np.array(isw, np.uint8),
                      np.array(val, np.uint64), status, len(att))
    invoke, complete = _attempt_intervals(att)
    return TxnOps(vh, int((status == TXN_OK).sum()), int((status == TXN_ABORTED).sum()),
                  sum(1 for a in att if a[2] == TXN_UNKNOWN and a[1] is not None),
                  sum(1 for a in att if a[1] is None), [a[1] if a[1] is not None else a[0] for a in att],
                  invoke, complete)


def vhistory_from_txn_edn(text: str) -> TxnOps:
    """Multi-op txn histories, ``{:f :txn :value [[:r k v] [:w k v] ...]}``
    (keys and values non-negative integers), as a value history of every
    attempted txn: a paired or unpaired op is a txn -- ``:ok`` is TXN_OK,
    ``:fail`` TXN_ABORTED, ``:info`` or an invoke without a completion
    TXN_UNKNOWN.  A ``nil`` read of an ``:ok`` op saw the initial state
    (VAL_INIT); the micro-ops of any other op come from its invoke, whose
    reads are ``nil`` and are left out."""
    att = _attempts(text, (":txn",))
    txn, key, isw, val = [], [], [], []
    for t, (inv, op, st, _, _) in enumerate(att):
        src = op if st == TXN_OK else (inv if ":value" in inv else (op or {}))
        for m in src.get(":value") or ():
            f, k, v = m
            if f == ":w":
                if v is None:
                    raise ValueError("a :w micro-op without a value")
                txn.append(t), key.append(int(k)), isw.append(1), val.append(int(v))
            elif f == ":r":
                if st != TXN_OK:
                    continue
                txn.append(t), key.append(int(k)), isw.append(0), val.append(VAL_INIT if v is None else int(v))
            else:
                raise ValueError(f"unknown micro-op {f!r}")
    return _txn_ops_record(att, txn, key, isw, val)


_RESOLVE_STATS = ("nops", "kept_ops", "ntxn", "ncommitted", "recovered", "aborted", "dropped", "writes", "reads",
                  "g1a_reads", "g1b_reads", "dangling_reads", "internal_reads", "g1a_txns", "g1b_txns",
                  "n_listed", "sweeps", "ms")
_RD_ABORTED, _RD_INTERMEDIATE, _RD_DANGLING = 1, 2, 4  # HSC_RD_*


def listed_reads(vh: ValueHistory, res: dict) -> dict:
    """``aborted_reads`` / ``intermediate_reads`` / ``dangling_reads`` of a
    dep_graph_resolve(arrays=True) dict: one entry {reader, writer, key,
    value, reader_op, writer_op} per listed read carrying the flag (writer
    and writer_op None for a dangling read), and the exact ``*_count`` of each
    (the lists stop at the entry's cap)."""
    out = {"aborted_reads": [], "intermediate_reads": [], "dangling_reads": []}
    for i, j in zip(res["listed_op"], res["listed_wop"]):
        i, j = int(i), int(j)
        none = j == 0xFFFFFFFFFFFFFFFF
        e = {"reader": int(vh.txn[i]), "writer": None if none else int(vh.txn[j]), "key": int(vh.key[i]),
             "value": int(vh.value[i]), "reader_op": i, "writer_op": None if none else j}
        f = int(res["rflag"][i])
        for bit, name in ((_RD_ABORTED, "aborted_reads"), (_RD_INTERMEDIATE, "intermediate_reads"),
                          (_RD_DANGLING, "dangling_reads")):
            if f & bit:
                out[name].append(e)
    out["aborted_read_count"] = int(res["g1a_reads"])
    out["intermediate_read_count"] = int(res["g1b_reads"])
    out["dangling_read_count"] = int(res["dangling_reads"])
    return out


# ---------------------------------------------------------------------------
# internal consistency (Elle's :internal): a txn's reads against its own ops
# ---------------------------------------------------------------------------
_INTERNAL_STATS = ("nops", "ntxn", "checked_reads", "bad_reads", "compared_elements", "bad_txns", "n_listed",
                   "sort_packed", "ms")
_INTERNAL_LEVELS = ("snapshot_isolation", "serializable", "strict_serializable", "strong_snapshot_isolation")


def _internal_keys(entries: list, res: dict) -> dict:
    return {"internal_anomalies": entries, "internal_anomaly_count": int(res["bad_reads"]),
            "internal": {k: res[k] for k in _INTERNAL_STATS if k in res}}


def internal_reads(vh: ValueHistory, res: dict) -> dict:
    """``internal_anomalies`` of a ``Validator.graph_internal`` dict (a pure
    function of its arguments): one entry {txn, key, op, anchor_op, expected,
    got} per listed bad read -- ``anchor_op`` the txn's previous op on the key
    and ``expected`` its value, ``got`` what the read returned (None for the
    initial state either way); the exact ``internal_anomaly_count`` (the list
    stops at the entry's cap) and ``internal``, the entry's scalar stats."""
    def val(i):
        v = int(vh.value[i])
        return None if v == VAL_INIT else v

    entries = [{"txn": int(vh.txn[i]), "key": int(vh.key[i]), "op": int(i), "anchor_op": int(a),
                "expected": val(int(a)), "got": val(int(i))}
               for i, a in zip(res["listed_op"], res["listed_anchor"])]
    return _internal_keys(entries, res)


def internal_list_reads(lh: ListHistory, res: dict) -> dict:
    """:func:`internal_reads` for a ``Validator.graph_internal_lists`` dict: one
    entry {txn, key, op, anchor_op, prefix, appended, got} per listed bad
    read -- ``prefix`` the list of the txn's previous read of the key
    (``anchor_op``), or None when there is none and ``anchor_op`` is the txn's
    first append to the key; ``appended`` the elements the txn appended to the
    key since; ``got`` the list the read returned, which should have been
    prefix + appended, or have ended in appended."""
    txn, key, isw = np.asarray(lh.txn), np.asarray(lh.key), np.asarray(lh.is_write)

    def lst(i):
        return [int(x) for x in lh.elems[int(lh.list_off[i]):int(lh.list_off[i + 1])]]

    entries = []
    for i, a in zip(res["listed_op"], res["listed_anchor"]):
        i, a = int(i), int(a)
        has_p = not isw[a]
        lo = a + 1 if has_p else a
        mine = np.nonzero((txn[lo:i] == txn[i]) & (key[lo:i] == key[i]) & (isw[lo:i] != 0))[0] + lo
        entries.append({"txn": int(txn[i]), "key": int(key[i]), "op": i, "anchor_op": a,
                        "prefix": lst(a) if has_p else None, "appended": [int(lh.value[j]) for j in mine],
                        "got": lst(i)})
    return _internal_keys(entries, res)


def with_internal(report: dict, keys: dict) -> dict:
    """A check_txn_edn / check_append_edn report with the keys of
    :func:`internal_reads` / :func:`internal_list_reads` merged in (a pure
    function: a new dict, ``levels`` copied): ``anomaly_types`` gains
    "internal" and ``valid`` turns False when there is a bad read; ``levels``,
    when the report has them, gains ``internal_consistent``, and every level
    present among snapshot_isolation, serializable, strict_serializable and
    strong_snapshot_isolation is and-ed with it -- the INT axiom is part of
    read atomic, which all four imply.  ``read_committed`` and ``g1c_free`` stay
    as they are: PL-2 says nothing about a txn's own writes."""
    out = dict(report)
    out.update(keys)
    ok = int(keys["internal_anomaly_count"]) == 0
    if not ok:
        out["anomaly_types"] = sorted(set(report["anomaly_types"]) | {"internal"})
        out["valid"] = False
    if "levels" in report:
        levels = dict(report["levels"])
        levels["internal_consistent"] = ok
        for name in _INTERNAL_LEVELS:
            if name in levels:
                levels[name] = bool(levels[name]) and ok
        out["levels"] = levels
    return out


def check_txn_edn(validator, text: str, witness: bool = True, realtime: bool = False,
                  isolation: bool = False, internal: bool = False) -> dict:
    """A multi-op txn history through the GPU by value: resolve every read to
    the write it observed (``Validator.dep_graph_resolve``), build the graph
    of the committed part (``dep_graph_build_resolved``) and run exactly the
    analyses of :func:`check_edn`.  The report has check_edn's keys -- the txns
    of ``cycles`` / ``si_cycles`` / ``realtime_cycles`` and their ``label``
    are attempted-txn ids (``history.txn_ops``), while ``analysis`` and its
    kin stay in committed ids, ``resolve_arrays["txn_of_cid"]`` mapping them
    -- plus :func:`listed_reads`' keys; ``anomaly_types`` gains "G1a" /
    "G1b"; ``valid`` = no cycle, no G1a and no G1b; ``levels`` (with
    ``isolation``) gains ``read_committed`` = no G1a, no G1b and
    ``g1c_free``; ``resolve`` holds the entry's stats, ``history`` the
    :class:`TxnOps`.  With ``realtime`` the intervals of the committed txns
    are staged; a recovered txn is open.

    ``internal``: also internal consistency (``Validator.graph_internal``, run
    right after the resolve on the history it uploaded): the report becomes
    :func:`with_internal`'s -- ``internal_anomalies``,
    ``internal_anomaly_count``, ``internal``, "internal" among
    ``anomaly_types``, ``valid`` False on any bad read, and with ``isolation``
    ``levels["internal_consistent"]`` and-ed into the levels from snapshot
    isolation up.  Without it internal consistency is not checked and the
    report is as it always was."""
    tx = vhistory_from_txn_edn(text)
    res = validator.dep_graph_resolve(tx.vhistory, arrays=True)
    own = internal_reads(tx.vhistory, validator.graph_internal()) if internal else None
    toc = [int(t) for t in res["txn_of_cid"]]
    sel = np.asarray(toc, np.int64)
    committed = TxnOps(tx.vhistory, tx.ok, tx.failed, tx.info, tx.unpaired, [tx.txn_ops[t] for t in toc],
                       tx.invoke[sel], tx.complete[sel])
    report = _check_built(validator, committed, lambda: validator.dep_graph_build_resolved(full=True),
                          len(toc), witness, realtime, isolation)
    for name in ("cycles", "si_cycles", "realtime_cycles"):
        for c in report.get(name, ()):
            c["txns"] = [toc[t] for t in c["txns"]]
            c["label"] = toc[c["label"]]
    report["history"] = tx
    report.update(listed_reads(tx.vhistory, res))
    g1a, g1b = int(res["g1a_reads"]) > 0, int(res["g1b_reads"]) > 0
    report["anomaly_types"] = sorted(set(report["anomaly_types"]) | ({"G1a"} if g1a else set())
                                     | ({"G1b"} if g1b else set()))
    report["valid"] = bool(report["valid"]) and not g1a and not g1b
    if isolation:
        report["levels"]["read_committed"] = not g1a and not g1b and bool(report["levels"]["g1c_free"])
    report["resolve"] = {k: res[k] for k in _RESOLVE_STATS if k in res}
    report["resolve_arrays"] = {k: res[k] for k in ("fate", "cid", "txn_of_cid", "txn_g1")}
    return report if own is None else with_internal(report, own)


# ---------------------------------------------------------------------------
# list-append histories: the version order comes from the reads
# ---------------------------------------------------------------------------
@dataclasses.dataclass
class AppendOps:
    """Every attempted txn of a list-append history, in txn id order (the
    fields of :class:`TxnOps`, the history a :class:`ListHistory`)."""
    lhistory: ListHistory
    ok: int
    failed: int
    info: int
    unpaired: int
    txn_ops: List[dict]
    invoke: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint64))
    complete: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, np.uint64))
    g2_keys: Dict[int, int] = dataclasses.field(default_factory=dict)  # (anomaly_report reads it: none here)


def lhistory_from_append_edn(text: str) -> AppendOps:
    """Elle's list-append histories, ``{:f :txn :value [[:append k v]
    [:r k [v ...]] ...]}`` (keys and elements non-negative integers), as a
    list history of every attempted txn: ``:ok`` is TXN_OK, ``:fail``
    TXN_ABORTED, ``:info`` or an invoke without a completion TXN_UNKNOWN.  A
    ``nil`` or ``[]`` read is the empty list.  An op that did not complete
    ``:ok`` gives its appends from the invoke and no reads.  Txn ids follow
    :func:`vhistory_from_txn_edn`'s order; nothing downstream relies on it."""
    att = _attempts(text, (":txn",))
    ops = []
    for t, (inv, op, st, _, _) in enumerate(att):
        src = op if st == TXN_OK else (inv if ":value" in inv else (op or {}))
        for m in src.get(":value") or ():
            f, k, v = m
            if f == ":append":
                if v is None:
                    raise ValueError("an :append micro-op without an element")
                ops.append((t, int(k), int(v)))
            elif f == ":r":
                if st == TXN_OK:
                    ops.append((t, int(k), [int(x) for x in (v or ())]))
            else:
                raise ValueError(f"unknown micro-op {f!r}")
    status = np.array([a[2] for a in att], np.uint8)
    invoke, complete = _attempt_intervals(att)
    return AppendOps(ListHistory.from_ops(ops, status), int((status == TXN_OK).sum()),
                     int((status == TXN_ABORTED).sum()),
                     sum(1 for a in att if a[2] == TXN_UNKNOWN and a[1] is not None),
                     sum(1 for a in att if a[1] is None), [a[1] if a[1] is not None else a[0] for a in att],
                     invoke, complete)


_LRESOLVE_STATS = ("nops", "ntxn", "ncommitted", "recovered", "aborted", "dropped", "appends", "reads", "elements",
                   "keys", "incompatible_keys", "spine_elements", "chain_entries", "ww", "wr", "rw", "g1a_reads",
                   "g1b_reads", "dangling_reads", "duplicate_reads", "incompatible_reads", "internal_reads",
                   "unobserved_appends", "g1a_txns", "g1b_txns", "n_listed", "ms")
_LRD_INCOMPATIBLE, _LRD_DUPLICATE = 16, 32  # HSC_LRD_*


def listed_list_reads(lh: ListHistory, res: dict) -> dict:
    """``aborted_reads`` / ``intermediate_reads`` / ``dangling_reads`` /
    ``duplicate_reads`` / ``incompatible_reads`` of a graph_resolve_lists
    dict: one entry {reader, key, reader_op, list} per listed read carrying the
    flag, and the exact ``*_count`` of each (the lists stop at the entry's
    cap)."""
    names = ((_RD_ABORTED, "aborted_reads"), (_RD_INTERMEDIATE, "intermediate_reads"),
             (_RD_DANGLING, "dangling_reads"), (_LRD_DUPLICATE, "duplicate_reads"),
             (_LRD_INCOMPATIBLE, "incompatible_reads"))
    out = {name: [] for _, name in names}
    for i, f in zip(res["listed_op"], res["listed_flag"]):
        i, f = int(i), int(f)
        e = {"reader": int(lh.txn[i]), "key": int(lh.key[i]), "reader_op": i,
             "list": [int(x) for x in lh.elems[int(lh.list_off[i]):int(lh.list_off[i + 1])]]}
        for bit, name in names:
            if f & bit:
                out[name].append(e)
    out["aborted_read_count"] = int(res["g1a_reads"])
    out["intermediate_read_count"] = int(res["g1b_reads"])
    out["dangling_read_count"] = int(res["dangling_reads"])
    out["duplicate_read_count"] = int(res["duplicate_reads"])
    out["incompatible_read_count"] = int(res["incompatible_reads"])
    return out


def check_append_edn(validator, text: str, witness: bool = True, realtime: bool = False,
                     isolation: bool = False, internal: bool = False) -> dict:
    """A list-append history through the GPU with no premise on commit order:
    the version order of every key is its longest read
    (``Validator.graph_resolve_lists``), the graph is built from the edges
    that order gives (``graph_build_lists``), and the analyses of
    :func:`check_edn` run on it.  Where :func:`check_txn_edn` must take
    completion order for version order -- and reports a false cycle, or misses
    one, when two concurrent writers of a key complete in the other order --
    this check reads the order the database applied from the data.

    The report has :func:`check_txn_edn`'s keys, the txns of ``cycles`` /
    ``si_cycles`` / ``realtime_cycles`` and their ``label`` mapped back to
    attempted-txn ids, plus :func:`listed_list_reads`' keys (``duplicate_reads``
    and ``incompatible_reads`` with their counts among them).
    ``anomaly_types`` gains "G1a", "G1b", "incompatible-order" (a read that is
    not a prefix of its key's longest read), "duplicate-elements" and "G0":
    a component whose witness cycle is made of ww edges only (its entry in
    ``cycles`` keeps the class ``type`` "G1c" and has ``g0`` True).  G0 is a
    lower bound: one witness is looked at per component, so a component may
    hold a ww-only cycle its witness does not show, and without ``witness``
    none is named.  ``valid`` = no cycle and none of the above; ``levels``
    (with ``isolation``) gains ``read_committed``.  ``resolve`` holds the
    entry's stats, ``history`` the :class:`AppendOps`.  A dangling read is
    listed and counted, and does not by itself make the history invalid, as
    in :func:`check_txn_edn`.

    ``internal``: also internal consistency (``Validator.graph_internal_lists``,
    run right after the resolve), reported as :func:`check_txn_edn` does with
    :func:`internal_list_reads`' entries.  Without it internal consistency is
    not checked and the report is as it always was."""
    tx = lhistory_from_append_edn(text)
    res = validator.graph_resolve_lists(tx.lhistory, arrays=True)
    own = internal_list_reads(tx.lhistory, validator.graph_internal_lists()) if internal else None
    toc = [int(t) for t in res["txn_of_cid"]]
    sel = np.asarray(toc, np.int64)
    committed = AppendOps(tx.lhistory, tx.ok, tx.failed, tx.info, tx.unpaired, [tx.txn_ops[t] for t in toc],
                          tx.invoke[sel], tx.complete[sel])
    report = _check_built(validator, committed, lambda: validator.graph_build_lists(full=True),
                          len(toc), witness, realtime, isolation)
    for name in ("cycles", "si_cycles", "realtime_cycles"):
        for c in report.get(name, ()):
            c["txns"] = [toc[t] for t in c["txns"]]
            c["label"] = toc[c["label"]]
    g0 = False
    for c in report["cycles"]:
        c["g0"] = bool(c["edge_types"]) and all(t == "ww" for t in c["edge_types"])
        g0 = g0 or c["g0"]
    report["history"] = tx
    report.update(listed_list_reads(tx.lhistory, res))
    extra = {name for name, k in (("G1a", "g1a_reads"), ("G1b", "g1b_reads"),
                                  ("incompatible-order", "incompatible_reads"),
                                  ("duplicate-elements", "duplicate_reads")) if int(res[k]) > 0}
    if g0:
        extra.add("G0")
    report["anomaly_types"] = sorted(set(report["anomaly_types"]) | extra)
    report["valid"] = bool(report["valid"]) and not extra
    if isolation:
        g1 = int(res["g1a_reads"]) > 0 or int(res["g1b_reads"]) > 0
        report["levels"]["read_committed"] = not g1 and bool(report["levels"]["g1c_free"])
    report["resolve"] = {k: res[k] for k in _LRESOLVE_STATS if k in res}
    report["resolve_arrays"] = {k: res[k] for k in ("fate", "cid", "txn_of_cid", "txn_g1")}
    return report if own is None else with_internal(report, own)


# ---- the reference's dirty-reads workload (core.clj:320-353, :492-523) ------
@dataclasses.dataclass
class DirtyOps:
    ops: TxnOps
    n: int              # rows
    short_reads: int    # :ok reads of fewer than n values (their positions are lost)
    reads: List[int]    # the txn ids of the :ok reads


def dirty_reads_from_edn(text: str, n: Optional[int] = None) -> DirtyOps:
    """The dirty-reads workload as a value history: ``:f :write :value x``
    writes x to rows 0 .. n - 1 in one txn; ``:f :read`` returns the x of
    every row that is not still initial, without row ids.  n defaults to the
    longest read (at least 1).  A read of n values maps position to key; a
    shorter one has lost its positions, and its values get keys 0 .. len - 1
    -- every write covers every row, so the (key, value) lookup, and with it
    G1a, stays exact while those keys mean nothing.  That is why this history
    is for the resolve alone, never for a graph."""
    att = _attempts(text, (":read", ":write"))
    f_of = [(op or inv).get(":f", inv.get(":f")) for inv, op, _, _, _ in att]
    vals_of = [list(op.get(":value") or ()) if f == ":read" and st == TXN_OK else None
               for f, (inv, op, st, _, _) in zip(f_of, att)]
    if n is None:
        n = max([1] + [len(v) for v in vals_of if v is not None])
    txn, key, isw, val, reads, short = [], [], [], [], [], 0
    for t, (f, (inv, op, st, _, _)) in enumerate(zip(f_of, att)):
        if f == ":write":
            x = inv.get(":value", (op or {}).get(":value"))
            for k in range(n):
                txn.append(t), key.append(k), isw.append(1), val.append(int(x))
        elif vals_of[t] is not None:
            vs = vals_of[t]
            if len(vs) > n:
                raise ValueError("a read of more values than rows")
            reads.append(t)
            short += len(vs) < n
            for k, x in enumerate(vs):
                txn.append(t), key.append(k), isw.append(0), val.append(int(x))
    return DirtyOps(_txn_ops_record(att, txn, key, isw, val), n, short, reads)


def dirty_reads_report(d: DirtyOps, res: dict) -> dict:
    """The dirty-reads checker's answer from a dep_graph_resolve dict (a pure
    function of its arguments): ``dirty_reads`` -- the values of the :ok reads
    holding a value of a :fail write, in txn order (the checker's docstring:
    "a failed transaction whose value became visible to some read");
    ``dirty_read_txns`` their txn ids; ``inconsistent_reads`` -- the reads
    whose values are not all equal (computed here, on the host); ``valid`` --
    no dirty read; ``short_reads``; ``resolve`` the entry's stats."""
    g1 = res["txn_g1"]
    dirty = [t for t in d.reads if int(g1[t]) & 1]
    values = {t: list(d.ops.txn_ops[t].get(":value") or ()) for t in d.reads}
    return {"valid": not dirty, "dirty_reads": [values[t] for t in dirty], "dirty_read_txns": dirty,
            "inconsistent_reads": [values[t] for t in d.reads if len(set(values[t])) > 1],
            "short_reads": d.short_reads, "n": d.n, "history": d,
            "resolve": {k: res[k] for k in _RESOLVE_STATS if k in res}}


def check_dirty_reads_edn(validator, text: str, n: Optional[int] = None) -> dict:
    """The reference's dirty-reads checker through the GPU: the resolve only
    (no graph: :func:`dirty_reads_from_edn`), then :func:`dirty_reads_report`."""
    d = dirty_reads_from_edn(text, n)
    return dirty_reads_report(d, validator.dep_graph_resolve(d.ops.vhistory, arrays=False))


# ---------------------------------------------------------------------------
# linearizability of register histories: a search, not a graph
# ---------------------------------------------------------------------------
LIN_READ, LIN_WRITE, LIN_CAS = 0, 1, 2   # hsc_linear_check's f
LIN_NIL = -(1 << 63)                     # HSC_LIN_NIL
LIN_BAD, LIN_OK, LIN_UNKNOWN = 0, 1, 2   # its verdicts
LIN_CAUSES = {0: None, 1: "slots", 2: "configs", 3: "budget", 4: "states"}
_LIN_F = {":read": LIN_READ, ":write": LIN_WRITE, ":cas": LIN_CAS}


@dataclasses.dataclass
class LinOps:
    """A register history as hsc_linear_check takes it: the ops that may have
    taken effect (``:ok``, and ``:info`` / unpaired as open ops)."""
    nkeys: int
    key: np.ndarray
    f: np.ndarray
    a: np.ndarray
    b: np.ndarray
    invoke: np.ndarray
    complete: np.ndarray
    keys: List[object]        # key index -> the history's key (None: the single register)
    completions: List[dict]   # per op: its completion as parsed (an unpaired op: its invoke)
    ok: int = 0
    failed: int = 0           # :fail completions (dropped with their invokes)
    info: int = 0
    unpaired: int = 0
    orphans: int = 0          # completions without an invoke (ignored)
    use_time: bool = False    # positions are ``:time`` (else line indices)

    def arrays(self) -> dict:
        """What ``Validator.linear_check`` takes."""
        return {k: getattr(self, k) for k in ("nkeys", "key", "f", "a", "b", "invoke", "complete")}


def lin_ops_from_register_edn(text: str, independent: bool = False) -> LinOps:
    """A knossos register history (``:f :read / :write / :cas``, no ``:uid``
    needed) -> :class:`LinOps`, by knossos' history completion
    (linearizable/jepsen/src/knossos/history.clj:87-171): invokes pair with
    their completions by ``:process``; an op that completes ``:fail`` never
    happened and is dropped, invoke included; an ``:ok`` op takes its value
    from the completion; an ``:info`` or unpaired op stays open with its
    invoke's value.  Keys: ``:key`` where an op carries one, the ``k`` of
    ``[k v]`` / ``[k [cur new]]`` values with ``independent`` (the reference's
    independent/tuple), else one register.  Positions are ``:time`` when every
    kept invoke and completion carries an integer one and every closed op's
    completion is later than its invoke, else line indices."""
    rows = []  # (invoke, completion or None, invoke line, completion line)
    pending: Dict[object, Tuple[dict, int]] = {}
    failed = orphans = 0
    for i, op in enumerate(_flatten(parse_edn(text))):
        if not isinstance(op, dict):
            continue
        t, p = op.get(":type"), op.get(":process")
        if t == ":invoke":
            if p in pending:
                rows.append(pending[p] + (None, -1))
            pending[p] = (op, i)
        elif t in (":ok", ":fail", ":info"):
            if p not in pending:
                orphans += 1
                continue
            inv, il = pending.pop(p)
            if t == ":fail":
                failed += 1
            else:
                rows.append((inv, il, op, i))
    rows += [v + (None, -1) for v in pending.values()]
    rows.sort(key=lambda r: r[1])
    closed = [r for r in rows if r[2] is not None and r[2].get(":type") == ":ok"]
    stamped = [o for inv, _, op, _ in rows for o in ((inv, op) if op is not None else (inv,))]
    use_time = (all(type(o.get(":time")) is int for o in stamped)
                and all(inv[":time"] < op[":time"] for inv, _, op, _ in closed))
    key_ix: Dict[object, int] = {}
    key, f, a, b, invoke, complete, comps = [], [], [], [], [], [], []
    n_ok = n_info = n_open = 0
    for inv, il, op, ol in rows:
        is_ok = op is not None and op.get(":type") == ":ok"
        fk = inv.get(":f")
        if fk not in _LIN_F:
            raise ValueError(f"not a register op: {fk!r}")
        val = op.get(":value", inv.get(":value")) if is_ok else inv.get(":value")
        k = inv.get(":key")
        if independent:
            k, val = val
        if fk == ":cas":
            cur, new = val
        else:
            cur, new = val, None
        key.append(key_ix.setdefault(k, len(key_ix)))
        f.append(_LIN_F[fk])
        a.append(LIN_NIL if cur is None else int(cur))
        b.append(LIN_NIL if new is None else int(new))
        invoke.append(inv[":time"] if use_time else il)
        complete.append(None if not is_ok else op[":time"] if use_time else ol)
        comps.append(op if op is not None else inv)
        n_ok += is_ok
        n_info += op is not None and not is_ok
        n_open += op is None
    base = min([0] + invoke)  # (a clock that starts below zero)
    return LinOps(len(key_ix), np.array(key, np.uint32), np.array(f, np.uint8), np.array(a, np.int64),
                  np.array(b, np.int64), np.array([t - base for t in invoke], np.uint64),
                  np.array([RT_OPEN if t is None else t - base for t in complete], np.uint64),
                  list(key_ix), comps, n_ok, failed, n_info, n_open, orphans, use_time)


def linear_report(ops: LinOps, res: dict) -> dict:
    """``Validator.linear_check``'s dict in the history's terms: ``valid``
    (True; False if a key is not linearizable; else "unknown" if a key's search
    passed a limit), ``keys`` -- per history key its ``verdict`` (True / False /
    "unknown"), ``cause`` ("slots" / "configs" for unknown), ``op`` (the
    completion whose return left no configuration), ``previous_ok`` (the key's
    last completion before it) and ``possible_values`` (what the register could
    hold before it; None = nil), ``peak_configs``, ``final_configs`` -- and the
    counts and ``ms``.  Of ``Validator.linear_check_wide``'s dict also each
    key's ``tier`` (1: judged by the wide tier; its cause may then be "budget"
    or "states") and ``escalated``, ``resolved``, ``wide_ms``."""
    names = {LIN_BAD: False, LIN_OK: True, LIN_UNKNOWN: "unknown"}
    keys = {}
    for k, name in enumerate(ops.keys):
        bad = res["verdict"][k] == LIN_BAD
        fo, po = int(res["fail_op"][k]), int(res["prev_ok"][k])
        keys[name] = {"verdict": names[int(res["verdict"][k])], "cause": LIN_CAUSES[int(res["cause"][k])],
                      "op": ops.completions[fo] if bad else None,
                      "previous_ok": ops.completions[po] if bad and po != 0xFFFFFFFF else None,
                      "possible_values": res["possible_values"][k] if bad else None,
                      "peak_configs": int(res["peak_configs"][k]), "final_configs": int(res["final_configs"][k])}
        if "tier" in res:
            keys[name]["tier"] = int(res["tier"][k])
    report = {"valid": False if res["bad"] else "unknown" if res["unknown"] else True, "keys": keys,
              "ok": ops.ok, "failed": ops.failed, "info": ops.info, "unpaired": ops.unpaired}
    report.update({k: res[k] for k in ("bad", "unknown", "events", "expanded", "dropped_open_reads", "ms")})
    if "tier" in res:
        report.update({k: res[k] for k in ("escalated", "resolved", "wide_ms")})
    return report


def check_linear_edn(validator, text: str, init=None, independent: bool = False, wide=False) -> dict:
    """knossos' checker/linearizable over cas-register-comdb2 through the GPU:
    :func:`lin_ops_from_register_edn`, ``Validator.linear_check``,
    :func:`linear_report` (plus ``history``, the :class:`LinOps`).  ``init``:
    the registers' initial value (None: nil), or a dict from history key to
    it.  ``wide``: True, or a dict of ``Validator.linear_check_wide``'s keyword
    arguments (``max_configs``, ``max_expanded``, ``arena_bytes``,
    ``wide_only``): the keys whose search leaves LDS are searched again in
    device memory instead of coming out "unknown"."""
    ops = lin_ops_from_register_edn(text, independent)
    if init is None:
        iv = None
    else:
        per = init if isinstance(init, dict) else {k: init for k in ops.keys}
        iv = np.array([LIN_NIL if per.get(k) is None else int(per[k]) for k in ops.keys], np.int64)
    if wide is False or wide is None:
        res = validator.linear_check(ops.arrays(), iv)
    else:
        res = validator.linear_check_wide(ops.arrays(), iv, **(wide if isinstance(wide, dict) else {}))
    report = linear_report(ops, res)
    report["history"] = ops
    return report


# ---------------------------------------------------------------------------
# the accounting checkers: set, total-queue, bank (no graph, no search)
# ---------------------------------------------------------------------------
TALLY_CLASSES = ("ok", "unexpected", "duplicated", "lost", "recovered")  # hsc_tally_check's classes


def _int_value(v, what: str) -> int:
    if type(v) is not int:
        raise ValueError(f"{what}: not an integer value: {v!r}")
    if not -(1 << 63) <= v < (1 << 63):
        raise ValueError(f"{what}: a value outside 64 bits: {v!r}")
    return v


def _typed_ops(text: str):
    """(type, f, op) of every op map, in history order (both layouts)."""
    for op in _flatten(parse_edn(text)):
        if isinstance(op, dict):
            yield op.get(":type"), op.get(":f"), op


@dataclasses.dataclass
class TallyOps:
    """The three value arrays ``Validator.tally_check`` takes.  ``seen`` is
    None for a set history without an ``:ok :read`` (or whose last one holds
    nil); ``read_op`` is that read's completion."""
    attempt: np.ndarray
    ack: np.ndarray
    seen: Optional[np.ndarray]
    read_op: Optional[dict] = None


def set_ops_from_edn(text: str) -> TallyOps:
    """checker/set's three collections (jepsen/checker.clj:114-128): the
    values of the ``:invoke :add`` ops, of the ``:ok :add`` ops, and the
    ``:value`` of the last ``:ok :read`` in history order.  Nothing is paired:
    a failed add is still an attempt, a completion without its invoke still an
    acknowledged add."""
    attempt, ack, last = [], [], None
    for t, f, op in _typed_ops(text):
        if f == ":add" and t == ":invoke":
            attempt.append(_int_value(op.get(":value"), "add"))
        elif f == ":add" and t == ":ok":
            ack.append(_int_value(op.get(":value"), "add"))
        elif f == ":read" and t == ":ok":
            last = op
    seen = None
    if last is not None and last.get(":value") is not None:
        vals = last[":value"]
        if not isinstance(vals, list):
            raise ValueError(f"read: not a collection: {vals!r}")
        seen = np.array([_int_value(v, "read") for v in vals], np.int64)
    return TallyOps(np.array(attempt, np.int64), np.array(ack, np.int64), seen, last)


def queue_ops_from_edn(text: str) -> TallyOps:
    """checker/total-queue's three multisets (jepsen/checker.clj:169-183): the
    values of ``:invoke :enqueue``, ``:ok :enqueue`` and ``:ok :dequeue``."""
    cols = {(":enqueue", ":invoke"): [], (":enqueue", ":ok"): [], (":dequeue", ":ok"): []}
    for t, f, op in _typed_ops(text):
        if (f, t) in cols:
            cols[(f, t)].append(_int_value(op.get(":value"), f[1:]))
    a, k, s = (np.array(v, np.int64) for v in cols.values())
    return TallyOps(a, k, s)


def interval_set_str(runs) -> str:
    """util/integer-interval-set-str (jepsen/util.clj:483-508) of the set whose
    runs of consecutive integers are ``runs`` [(lo, hi), ...], ascending:
    ``#{0..5 7 9..11}``."""
    return "#{" + " ".join(str(int(lo)) if lo == hi else f"{int(lo)}..{int(hi)}" for lo, hi in runs) + "}"


def _frac(count: int, attempts: int):
    return fractions.Fraction(count, attempts) if attempts else fractions.Fraction(1)


def _class_runs(res: dict, name: str) -> List[Tuple[int, int, int]]:
    c = res[name]
    return [(int(lo), int(hi), int(m)) for lo, hi, m in zip(c["lo"], c["hi"], c["mult"])]


def _truncated(res: dict) -> List[str]:
    return [c for c in TALLY_CLASSES if res[c]["runs"] > res[c]["n_listed"]]


def set_report(ops: TallyOps, res: Optional[dict]) -> dict:
    """checker/set's answer (jepsen/checker.clj:129-154) from a
    ``Validator.tally_check`` dict of ``ops`` in set mode (a pure function of
    its arguments; ``res`` is not looked at when the set was never read):
    ``valid``; ``ok`` / ``lost`` / ``unexpected`` / ``recovered`` as the
    reference's interval strings, built from the listed runs; ``*_count``;
    ``*_frac`` over the attempts (1 when there are none); ``truncated`` -- the
    classes with more runs than the entry lists, whose strings stop early;
    ``tally`` -- the entry's dict."""
    if ops.seen is None:
        return {"valid": "unknown", "error": "Set was never read"}
    report = {"valid": bool(res["valid"]), "truncated": _truncated(res), "tally": res}
    for c in ("ok", "lost", "unexpected", "recovered"):
        report[c] = interval_set_str((lo, hi) for lo, hi, _ in _class_runs(res, c))
        report[c + "_count"] = int(res[c]["count"])
        report[c + "_frac"] = _frac(int(res[c]["count"]), int(res["attempts"]))
    return report


def check_set_edn(validator, text: str) -> dict:
    """checker/set through the GPU: :func:`set_ops_from_edn`,
    ``Validator.tally_check``, :func:`set_report`.  A history without an
    ``:ok :read`` makes no GPU call."""
    ops = set_ops_from_edn(text)
    if ops.seen is None:
        return set_report(ops, None)
    return set_report(ops, validator.tally_check(ops.attempt, ops.ack, ops.seen))


def total_queue_report(ops: TallyOps, res: dict) -> dict:
    """checker/total-queue's answer (jepsen/checker.clj:184-218) from a
    ``Validator.tally_check`` dict of ``ops`` in multiset mode (a pure
    function): ``valid`` -- no lost and no unexpected; the five classes as run
    lists ``[(lo, hi, mult), ...]`` (mult copies of every integer lo .. hi);
    ``*_count``, ``*_frac``, ``truncated``, ``tally``."""
    report = {"valid": bool(res["valid"]), "truncated": _truncated(res), "tally": res}
    for c in TALLY_CLASSES:
        report[c] = _class_runs(res, c)
        report[c + "_count"] = int(res[c]["count"])
        report[c + "_frac"] = _frac(int(res[c]["count"]), int(res["attempts"]))
    return report


def check_total_queue_edn(validator, text: str) -> dict:
    """checker/total-queue through the GPU: :func:`queue_ops_from_edn`,
    ``Validator.tally_check(multiset=True)``, :func:`total_queue_report`."""
    ops = queue_ops_from_edn(text)
    return total_queue_report(ops, validator.tally_check(ops.attempt, ops.ack, ops.seen, multiset=True))


@dataclasses.dataclass
class BankOps:
    """The ``:ok :read`` ops of a bank history in CSR form, as
    ``Validator.bank_check`` takes them, and their completions."""
    off: np.ndarray
    balance: np.ndarray
    completions: List[dict]


def bank_ops_from_edn(text: str) -> BankOps:
    """bank-checker's reads (core.clj:157-161): the balances of every
    ``:ok :read`` in history order."""
    off, bal, comps = [0], [], []
    for t, f, op in _typed_ops(text):
        if t != ":ok" or f != ":read":
            continue
        vals = op.get(":value")
        if not isinstance(vals, list):
            raise ValueError(f"read: not a collection of balances: {vals!r}")
        bal.extend(_int_value(v, "read") for v in vals)
        off.append(len(bal))
        comps.append(op)
    return BankOps(np.array(off, np.uint64), np.array(bal, np.int64), comps)


_BANK_KINDS = {1: "wrong-n", 2: "wrong-total"}


def bank_report(ops: BankOps, res: dict, n: int, total: int) -> dict:
    """bank-checker's answer (core.clj:162-177) from a ``Validator.bank_check``
    dict (a pure function): ``valid``; ``bad_reads`` -- for the listed bad
    reads in history order ``{"type": "wrong-n" | "wrong-total", "expected",
    "found", "op"}``; ``bad_read_count``, ``wrong_n``, ``wrong_total``;
    ``negative_reads`` -- reads holding a negative balance, which the
    reference's checker does not judge and ``valid`` does not count;
    ``truncated`` -- more bad reads than listed; ``bank`` -- the entry's dict."""
    bad = []
    for i in res["listed_read"]:
        k = int(res["kind"][int(i)])
        bad.append({"type": _BANK_KINDS[k], "expected": n if k == 1 else total, "found": int(res["found"][int(i)]),
                    "op": ops.completions[int(i)]})
    return {"valid": bool(res["valid"]), "bad_reads": bad, "bad_read_count": int(res["bad"]),
            "wrong_n": int(res["wrong_n"]), "wrong_total": int(res["wrong_total"]),
            "negative_reads": int(res["reads_with_negative"]), "truncated": res["bad"] > res["n_listed"],
            "bank": res}


def check_bank_edn(validator, text: str, n: int, total: int) -> dict:
    """bank-checker through the GPU: :func:`bank_ops_from_edn`,
    ``Validator.bank_check``, :func:`bank_report`.  ``n`` and ``total`` are the
    test's ``:model`` (accounts, the sum of their starting balances)."""
    ops = bank_ops_from_edn(text)
    return bank_report(ops, validator.bank_check(ops.off, ops.balance, n, total), n, total)


# ---------------------------------------------------------------------------
# checker/perf (latencies, latency quantiles, rates) and checker/compose
# ---------------------------------------------------------------------------
PERF_TYPES = (":invoke", ":ok", ":fail", ":info")  # HSC_OP_INVOKE ..
PERF_GRAPH_TYPES = (":ok", ":info", ":fail")       # perf.clj:158-160, the order the graphs list them in
PERF_ALL = ":jepsen.checker.perf/all"              # perf.clj's ::all
_DEC64 = decimal.Context(prec=16, rounding=decimal.ROUND_HALF_EVEN)


def _poly_key(v):
    """A sort key that orders like util/poly-compare (jepsen/util.clj:471-481):
    ``compare`` inside one class (nil first), the class names across classes."""
    if v is None:
        return (0, "", "")
    if isinstance(v, bool):
        return (1, "class java.lang.Boolean", v)
    if isinstance(v, int):
        return (1, "class java.lang.Long", v)
    if isinstance(v, str):
        return (1, "class clojure.lang.Keyword" if v.startswith(":") else "class java.lang.String", v)
    raise ValueError(f"an :f the perf checker cannot order: {v!r}")


def nanos_to_ms(ns: int) -> float:
    """``(double (util/nanos->ms ns))`` (jepsen/util.clj:216, perf.clj:134): the
    ratio ns / 1000000 as a double.  Clojure converts a ratio through 16
    decimal digits (``Ratio.doubleValue``), which is the correctly rounded
    quotient for every |ns| below 10^16."""
    ns = int(ns)
    if abs(ns) < 10 ** 16 or ns % 1000000 == 0:
        return ns / 1000000
    return float(_DEC64.divide(decimal.Decimal(ns), decimal.Decimal(1000000)))


def bucket_of(t_ns: int, dt) -> int:
    """The window of a time under ``dt`` seconds: perf.clj:15-25 after
    util/nanos->secs, two double divisions, truncated."""
    return int((int(t_ns) / 1e9) / dt)


def bucket_mid(b: int, dt):
    """bucket-scale (perf.clj:15-19): the window's midpoint in seconds."""
    return b * dt + dt / 2


@dataclasses.dataclass
class PerfOps:
    """A timed history as ``Validator.perf_check`` takes it: one row per op in
    history order.  ``fs`` / ``processes``: what the ``f`` / ``process`` ids
    stand for (``fs`` in util/polysort order); ``nemesis``: the (:f, time) of
    the ``:process :nemesis`` ops in history order."""
    type: np.ndarray
    f: np.ndarray
    process: np.ndarray
    client: np.ndarray
    time: np.ndarray
    fs: List
    processes: List
    nemesis: List[Tuple[object, int]]


def perf_ops_from_edn(text: str) -> PerfOps:
    """Interns ``:f`` and ``:process`` of every op map.  Raises ValueError for
    an op without an integer ``:time`` (the reference throws there too: a
    NullPointerException in util/history->latencies) or a ``:type`` that is
    none of PERF_TYPES."""
    rows = []
    for i, op in enumerate(o for o in _flatten(parse_edn(text)) if isinstance(o, dict)):
        t = op.get(":time")
        if type(t) is not int or not 0 <= t < (1 << 63):
            raise ValueError(f"op {i}: no integer :time in [0, 2^63): {t!r}")
        if op.get(":type") not in PERF_TYPES:
            raise ValueError(f"op {i}: :type {op.get(':type')!r}")
        p = op.get(":process")
        if isinstance(p, (list, dict)):
            raise ValueError(f"op {i}: :process {p!r}")
        rows.append((PERF_TYPES.index(op[":type"]), op.get(":f"), p, t))
    fs = sorted({r[1] for r in rows}, key=_poly_key)
    fid = {v: k for k, v in enumerate(fs)}
    pid: Dict[object, int] = {}
    for r in rows:
        pid.setdefault((type(r[2]), r[2]), len(pid))
    n = len(rows)
    return PerfOps(np.fromiter((r[0] for r in rows), np.uint8, n), np.fromiter((fid[r[1]] for r in rows), np.uint32, n),
                   np.fromiter((pid[(type(r[2]), r[2])] for r in rows), np.uint32, n),
                   np.fromiter((type(r[2]) is int for r in rows), np.uint8, n),
                   np.fromiter((r[3] for r in rows), np.int64, n), fs, [k[1] for k in pid],
                   [(r[1], r[3]) for r in rows if r[2] == ":nemesis"])


def nemesis_intervals(nemesis, last_time: Optional[int]) -> List[Tuple[float, float]]:
    """perf.clj:168-187 over util/nemesis-intervals (jepsen/util.clj:589-606):
    ``nemesis`` = the (:f, time ns) of the nemesis ops in history order.  A
    ``:stop`` closes the oldest open ``:start`` (a queue: start start stop stop
    pairs first with third, second with fourth); a stop with no start open is
    dropped; a start never stopped ends at ``last_time``, the history's last
    time.  [(start s, stop s), ...]: the closed ones in stop order, then the
    open ones."""
    pairs, starts = [], []
    for f, t in nemesis:
        if f == ":start":
            starts.append(t)
        elif f == ":stop":
            pairs.append((starts.pop(0) if starts else None, t))
    pairs += [(t, None) for t in starts]
    return [(a / 1e9, (last_time if b is None else b) / 1e9) for a, b in pairs if a is not None]


def perf_report(ops: PerfOps, res: dict) -> dict:
    """checker/perf's data sets from a ``Validator.perf_check`` dict of ``ops``
    (a pure function of its arguments; the windows and quantiles are the
    ``q_dt``, ``r_dt`` and ``qs`` the dict echoes):

    ``valid``: True (checker.clj:295, :303).  ``latency_raw`` (only when the
    dict has the arrays): {f: {":ok" | ":info" | ":fail": [(seconds, ms), ...]}}
    in history order, for every f with an invoke (perf.clj:96-102, :129-134).
    ``latency_quantiles``: {f: {q: [(window midpoint s, ms), ...]}} by window
    (perf.clj:45-79, :246-260).  ``rate``: {f: {type: [(midpoint, hz), ...]}}
    as rate-graph! emits it (perf.clj:293-331): for every f with a client
    completion and each of PERF_GRAPH_TYPES the series over the midpoints <=
    t-max, 0 where no op fell, a value being 1/dt added once per op (not count
    / dt); a completion in a last, partly filled window whose midpoint lies
    past t-max is therefore not in the series.  ``counts``: perf.clj:113-127's
    map {f: {type: n, PERF_ALL: n}, PERF_ALL: {...}} over every op that is no
    invoke.  ``nemesis_intervals``: :func:`nemesis_intervals`.  The scalars
    ``n``, ``invokes``, ``paired``, ``unpaired``, ``orphans``, ``t_max``,
    ``cells``, ``rate_cells``; ``truncated``: the data sets ("latency_quantiles",
    "rate") with more cells than the entry lists; ``perf``: the entry's dict.

    Unpaired invokes -- an invoke whose process invoked again first, or that
    never completed: the reference cannot plot a history with one
    (latency-point divides nil).  Here they are left out of every data set and
    counted in ``unpaired``."""
    qs, q_dt, r_dt = list(res["qs"]), res["q_dt"], res["r_dt"]
    fs = ops.fs
    invoked = np.bincount(ops.f[ops.type == 0], minlength=len(fs)) if len(ops.f) else np.zeros(len(fs), np.int64)
    report = {"valid": True}
    if "raw_op" in res:
        raw = {}
        off = res["raw_off"]
        for k, f in enumerate(fs):
            if not invoked[k]:
                continue
            raw[f] = {}
            for t in PERF_GRAPH_TYPES:
                g = k * 4 + PERF_TYPES.index(t)
                idx = res["raw_op"][int(off[g]):int(off[g + 1])]
                raw[f][t] = [(int(ops.time[i]) / 1e9, nanos_to_ms(res["latency"][i])) for i in idx]
        report["latency_raw"] = raw
    quant = {f: {q: [] for q in qs} for k, f in enumerate(fs) if invoked[k]}
    for k in range(int(res["cells_listed"])):
        f = fs[int(res["cell_f"][k])]
        mid = bucket_mid(int(res["cell_bucket"][k]), q_dt)
        for j, q in enumerate(qs):
            quant[f][q].append((mid, nanos_to_ms(res["cell_lat"][k][j])))
    report["latency_quantiles"] = quant
    # rate: 1 / dt added count times, sequentially, as the reduce of perf.clj:304-311 does
    td = 1.0 / r_dt  # (double (/ dt)), perf.clj:297
    most = int(res["rate_count"].max()) if len(res["rate_count"]) else 0
    hz = np.concatenate([[0.0], np.cumsum(np.full(most, td))])  # (numpy's cumsum adds in order)
    t_max = int(res["t_max"]) / 1e9
    mids = []
    while bucket_mid(len(mids), r_dt) <= t_max:
        mids.append(bucket_mid(len(mids), r_dt))
    rate = {}
    for f_, t_, b_, c_ in zip(res["rate_f"], res["rate_type"], res["rate_bucket"], res["rate_count"]):
        if fs[int(f_)] not in rate:
            rate[fs[int(f_)]] = {t: [0] * len(mids) for t in PERF_GRAPH_TYPES}
        series = rate[fs[int(f_)]]
        if int(b_) < len(mids):
            series[PERF_TYPES[int(t_)]][int(b_)] = float(hz[int(c_)])
    report["rate"] = {f: {t: list(zip(mids, v)) for t, v in d.items()} for f, d in rate.items()}
    counts: Dict = {}
    for k, f in enumerate(fs):
        for t in (1, 2, 3):
            c = int(res["counts"][k][t])
            if c:
                for a, b in ((f, PERF_TYPES[t]), (f, PERF_ALL), (PERF_ALL, PERF_TYPES[t]), (PERF_ALL, PERF_ALL)):
                    counts.setdefault(a, {})
                    counts[a][b] = counts[a].get(b, 0) + c
    report["counts"] = counts
    report["nemesis_intervals"] = nemesis_intervals(ops.nemesis, int(ops.time[-1]) if len(ops.time) else None)
    for k in ("n", "invokes", "paired", "unpaired", "orphans", "t_max", "cells", "rate_cells"):
        report[k] = int(res[k])
    report["truncated"] = [name for name, a, b in (("latency_quantiles", "cells", "cells_listed"),
                                                   ("rate", "rate_cells", "rate_listed")) if res[a] > res[b]]
    report["perf"] = res
    return report


def check_perf_edn(validator, text: str, arrays: bool = False, **windows) -> dict:
    """checker/perf through the GPU: :func:`perf_ops_from_edn`,
    ``Validator.perf_check``, :func:`perf_report`.  ``windows``: ``qs``,
    ``q_dt``, ``r_dt`` of ``perf_check``; ``arrays``: also ``latency_raw``."""
    ops = perf_ops_from_edn(text)
    res = validator.perf_check(ops.type, ops.f, ops.process, ops.client, ops.time, max(len(ops.fs), 1),
                               arrays=arrays, **windows)
    return perf_report(ops, res)


def with_times(text: str, seed: int, mean_latency_ns: int = 1_000_000, nemesis=()) -> str:
    """The EDN history ``text`` (one op map per line, as the generators here
    write them, which carry no ``:time``) with strictly increasing integer
    ``:time`` s stamped on its lines: the gaps are 1 + exponential with mean
    ``mean_latency_ns`` divided by the number of processes seen, so that an
    op's latency comes to about ``mean_latency_ns``.  ``nemesis``: (line, "start"
    | "stop") pairs; before that line of ``text`` the nemesis's two ``:info``
    ops of that ``:f`` are spliced in, as Jepsen logs a nemesis action."""
    rng = np.random.default_rng(seed)
    lines = [ln for ln in text.split("\n") if ln.strip()]
    procs = len(set(re.findall(r":process (\S+?)[,}]", text))) or 1
    splice: Dict[int, List[str]] = {}
    for at, what in nemesis:
        if what not in ("start", "stop"):
            raise ValueError(f"nemesis: {what!r}")
        splice.setdefault(min(max(int(at), 0), len(lines)), []).extend(
            [f"{{:type :info, :f :{what}, :process :nemesis, :value nil}}"] * 2)
    out, t = [], 0
    for i in range(len(lines) + 1):
        for ln in splice.get(i, []) + (lines[i:i + 1]):
            ln = ln.rstrip()
            if not ln.endswith("}"):
                raise ValueError(f"line {i}: not one op map per line")
            t += 1 + int(rng.exponential(mean_latency_ns / procs))
            out.append(f"{ln[:-1]}, :time {t}}}")
    return "\n".join(out) + "\n"


_VALID_PRIORITIES = ((True, 0), ("unknown", 0.5), (False, 1))  # checker.clj:20-25


def merge_valid(valids):
    """merge-valid (checker.clj:27-35): of True, "unknown" and False the one of
    the highest priority (True 0, "unknown" 0.5, False 1).  Raises ValueError
    for no values or a value that is none of the three."""
    def priority(v):
        for name, p in _VALID_PRIORITIES:
            if v is name or (isinstance(v, str) and v == name):
                return p
        raise ValueError(f"not a :valid? value: {v!r}")
    valids = list(valids)
    if not valids:
        raise ValueError("merge_valid of nothing")
    best = valids[0]
    priority(best)
    for v in valids[1:]:
        if priority(best) < priority(v):
            best = v
    return best


def compose_edn(validator, text: str, checkers: dict) -> dict:
    """checker/compose (checker.clj:274-286): runs every ``checkers[name]
    (validator, text)`` on the history and returns {name: its report, ...,
    "valid": :func:`merge_valid` of the reports' ``valid``}.  A member that
    raises gives {"valid": "unknown", "error": the exception's text}, as
    check-safe does (checker.clj:54-64).  A key that
    :func:`check_linear_edn` leaves undecided makes its report, and so the
    composition unless another member is invalid, "unknown".

    The presets are the compositions of core.clj whose members exist
    unambiguously here: COMPOSE_SETS (:269-271), COMPOSE_REGISTER (:585-587,
    :610-612) and :func:`compose_bank` (:291-294, :313-316).  core.clj also
    lists an ``independent`` linearizable member for its bank and dirty-reads
    tests; the presets leave it out, a caller may add it."""
    results = {}
    for name, check in checkers.items():
        try:
            results[name] = check(validator, text)
        except Exception as e:  # noqa: BLE001  (check-safe catches Throwable)
            results[name] = {"valid": "unknown", "error": f"{type(e).__name__}: {e}"}
    results["valid"] = merge_valid(r["valid"] for r in list(results.values()))
    return results


COMPOSE_SETS = {"perf": check_perf_edn, "set": check_set_edn}
COMPOSE_REGISTER = {"perf": check_perf_edn, "linearizable": check_linear_edn}


def compose_bank(n: int, total: int) -> dict:
    """The bank tests' composition for the model (n accounts, total)."""
    return {"perf": check_perf_edn, "bank": lambda v, text: check_bank_edn(v, text, n, total)}


# ---------------------------------------------------------------------------
# the counter and queue checkers, per independent key
# ---------------------------------------------------------------------------
CNT_NIL = -(1 << 63)                              # HSC_CNT_NIL
_CNT_F = {":add": 0, ":read": 1}                  # HSC_CNT_ADD, HSC_CNT_READ; anything else HSC_CNT_OTHER
_CNT_VALID = {0: True, 1: False, 2: "unknown"}    # HSC_CNT_OK / _BAD / _UNKNOWN
_CNT_KINDS = {1: "the process already has an op running", 2: "a completion without a prior invocation",
              3: "the failure's value differs from its invocation's",
              4: "the completion's :f differs from its invocation's",
              5: "a nil value where the counter needs a number"}


@dataclasses.dataclass
class KeyedRows:
    """Rows of a history as ``Validator.counter_check`` / ``queue_check`` take
    them.  ``keys``: key index -> the history's key (None: the single
    subhistory); ``ops``: per row its op as parsed."""
    nkeys: int
    key: np.ndarray
    f: np.ndarray
    value: np.ndarray
    keys: List[object]
    ops: List[dict]
    type: Optional[np.ndarray] = None
    process: Optional[np.ndarray] = None


def _unwrap(op: dict, i: int, independent: bool):
    """(key, value, keep) of an op: with ``independent`` the ``[k v]`` tuple of
    independent/tuple unwrapped as :func:`lin_ops_from_register_edn` does.  The
    reference puts an un-keyed op into every subhistory
    (jepsen/independent.clj:239-250); an ``:info`` one changes nothing in
    either checker and is dropped, any other is a ValueError."""
    v = op.get(":value")
    if not independent:
        return None, v, True
    if isinstance(v, list) and len(v) == 2:
        k = v[0]
        return (tuple(k) if isinstance(k, list) else k), v[1], True
    if op.get(":type") == ":info":
        return None, None, False
    raise ValueError(f"op {i}: an un-keyed op in an independent history: {op!r}")


def counter_ops_from_edn(text: str, independent: bool = False) -> KeyedRows:
    """Every op map of a counter history as a row: ``:type``, ``:f`` (``:add``
    / ``:read`` / other), ``:process`` interned, ``:value`` (nil -> CNT_NIL; a
    value of an other-f op that is no integer is interned too: only its
    equality with its invocation's matters)."""
    key_ix: Dict[object, int] = {}
    pid: Dict[object, int] = {}
    odd: Dict[str, int] = {}
    key, typ, f, proc, val, ops = [], [], [], [], [], []
    for i, op in enumerate(o for o in _flatten(parse_edn(text)) if isinstance(o, dict)):
        if op.get(":type") not in PERF_TYPES:
            raise ValueError(f"op {i}: :type {op.get(':type')!r}")
        k, v, keep = _unwrap(op, i, independent)
        if not keep:
            continue
        fk = _CNT_F.get(op.get(":f"), 2)
        if v is None:
            v = CNT_NIL
        elif fk == 2 and type(v) is not int:
            v = (1 << 62) + odd.setdefault(repr(v), len(odd))
        else:
            v = _int_value(v, "counter")
        p = op.get(":process")
        key.append(key_ix.setdefault(k, len(key_ix)))
        typ.append(PERF_TYPES.index(op[":type"]))
        f.append(fk)
        proc.append(pid.setdefault((type(p), repr(p)), len(pid)))
        val.append(v)
        ops.append(op)
    return KeyedRows(max(len(key_ix), 1), np.array(key, np.uint32), np.array(f, np.uint8), np.array(val, np.int64),
                     list(key_ix) or [None], ops, np.array(typ, np.uint8), np.array(proc, np.uint32))


def _independent(rows: KeyedRows, reports: List[dict], independent: bool) -> dict:
    """One report, or independent/checker's map of them
    (jepsen/independent.clj:252-290)."""
    if not independent:
        return reports[0]
    results = {} if rows.keys == [None] and not rows.ops else dict(zip(rows.keys, reports))
    return {"valid": merge_valid(r["valid"] for r in results.values()) if results else True, "results": results,
            "failures": [k for k, r in results.items() if r["valid"] is not True]}


def counter_report(rows: KeyedRows, res: dict, independent: bool = False) -> dict:
    """checker/counter's map per key from a ``Validator.counter_check`` dict (a
    pure function): {"valid", "reads": [[lower, value, upper], ...],
    "errors": [...]}, or {"valid": "unknown", "error": ...} naming the op of a
    malformed history (the reference throws there; check-safe answers
    :unknown)."""
    reports = []
    for k in range(rows.nkeys):
        if res["verdict"][k] == 2:
            o, kind = int(res["malformed_op"][k]), int(res["malformed_kind"][k])
            reports.append({"valid": "unknown", "op": rows.ops[o], "op_index": o, "kind": kind,
                            "error": f"malformed history at op {o} ({_CNT_KINDS[kind]}): {rows.ops[o]!r}"})
            continue
        a, b = int(res["read_off"][k]), int(res["read_off"][k + 1])
        reads = [[int(lo), int(v), int(hi)] for lo, v, hi in
                 zip(res["lower"][a:b], res["value"][a:b], res["upper"][a:b])]
        reports.append({"valid": _CNT_VALID[int(res["verdict"][k])], "reads": reads,
                        "errors": [r for r in reads if not r[0] <= r[1] <= r[2]]})
    return _independent(rows, reports, independent)


def check_counter_edn(validator, text: str, independent: bool = False) -> dict:
    """checker/counter (jepsen/checker.clj:220-272) through the GPU --
    wrapped in independent/checker with ``independent`` --
    :func:`counter_ops_from_edn`, ``Validator.counter_check``,
    :func:`counter_report`."""
    rows = counter_ops_from_edn(text, independent)
    res = validator.counter_check(rows.type, rows.f, rows.process, rows.value, rows.key, rows.nkeys)
    return counter_report(rows, res, independent)


def queue_rows_from_edn(text: str, independent: bool = False) -> KeyedRows:
    """The rows checker/queue selects (jepsen/checker.clj:95-100), in history
    order: every ``:invoke :enqueue`` and every ``:ok :dequeue``."""
    key_ix: Dict[object, int] = {}
    key, f, val, ops = [], [], [], []
    for i, op in enumerate(o for o in _flatten(parse_edn(text)) if isinstance(o, dict)):
        k, v, keep = _unwrap(op, i, independent)
        if not keep:
            continue
        tf = (op.get(":type"), op.get(":f"))
        if independent:
            key_ix.setdefault(k, len(key_ix))  # (a key with no selected row still has a subhistory)
        if tf not in ((":invoke", ":enqueue"), (":ok", ":dequeue")):
            continue
        key.append(key_ix.setdefault(k, len(key_ix)))
        f.append(0 if tf[1] == ":enqueue" else 1)
        val.append(_int_value(v, tf[1][1:]))
        ops.append(op)
    return KeyedRows(max(len(key_ix), 1), np.array(key, np.uint32), np.array(f, np.uint8), np.array(val, np.int64),
                     list(key_ix) or [None], ops)


def queue_report(rows: KeyedRows, res: dict, fifo: bool, independent: bool = False) -> dict:
    """checker/queue's map per key from a ``Validator.queue_check(final=True)``
    dict (a pure function): {"valid": True, "final_queue": ...} -- unordered:
    the remaining (value, multiplicity) pairs ascending; fifo: the remaining
    values in queue order -- or {"valid": False, "error": msg} with the
    model's message (jepsen/model.clj:80, :93-100)."""
    reports = []
    for k in range(rows.nkeys):
        if res["verdict"][k]:
            r = int(res["error_row"][k])
            msg = f"can't dequeue {int(rows.value[r])}" + (" from empty queue" if res["error_kind"][k] == 2 else "")
            reports.append({"valid": False, "error": msg, "op": rows.ops[r]})
            continue
        a, b = int(res["final_off"][k]), int(res["final_off"][k + 1])
        vals = [int(v) for v in res["final_val"][a:b]]
        reports.append({"valid": True, "final_queue": vals if fifo else
                        list(zip(vals, (int(m) for m in res["final_mult"][a:b])))})
    return _independent(rows, reports, independent)


def check_queue_edn(validator, text: str, model: str = "unordered", independent: bool = False) -> dict:
    """checker/queue (jepsen/checker.clj:87-106) through the GPU with the
    ``model`` "unordered" (model/unordered-queue) or "fifo" (model/fifo-queue),
    wrapped in independent/checker with ``independent``."""
    if model not in ("unordered", "fifo"):
        raise ValueError(f"model: {model!r}")
    rows = queue_rows_from_edn(text, independent)
    res = validator.queue_check(rows.f, rows.value, rows.key, rows.nkeys, fifo=model == "fifo", final=True)
    return queue_report(rows, res, model == "fifo", independent)


# ---------------------------------------------------------------------------
# generated histories (test inputs; the reference's clients need a live
# cluster and a JVM)
# ---------------------------------------------------------------------------
def register_history_edn(seed: int, n_ops: int = 2000, n_procs: int = 8, n_keys: int = 1,
                         lost_update: float = 0.02, stale_read: float = 0.05,
                         fail: float = 0.05) -> Tuple[str, int]:
    """A register.c-shaped history (read / write / cas, values rand() % 5,
    uids rand() % 100000) of a serial execution with injected anomalies:
    ``lost_update`` -- a cas whose ``cur`` is the value of an older version
    than the latest (both 'saw' it: a cycle with the writer in between);
    ``stale_read`` -- a read returning an older version.  Completions are
    logged in commit order, each op's invoke at a random earlier time (ops
    of one process never overlap).  n_keys > 1 adds ``:key`` (independent
    registers).  Returns (EDN text, injected lost updates)."""
    rng = np.random.default_rng(seed)
    versions: Dict[int, List[Tuple[int, int]]] = {k: [] for k in range(1, n_keys + 1)}
    lines: List[Tuple[int, int, str]] = []
    busy = np.zeros(n_procs, np.int64)
    now, lost = 1000, 0
    for _ in range(n_ops):
        now += int(rng.integers(1, 50))
        p = int(rng.integers(0, n_procs))
        inv_t = max(int(busy[p]) + 1, now - int(rng.integers(0, 400)))
        k = int(rng.integers(1, n_keys + 1))
        kk = f" :key {k}" if n_keys > 1 else ""
        vs = versions[k]
        op = int(rng.integers(0, 3))
        uid = int(rng.integers(0, 100000))
        new = int(rng.integers(0, 5))
        ok = rng.random() >= fail
        if op == 0:
            inv = f"{{:type :invoke :f :read :value nil :process {p}{kk} :time {inv_t}}}"
            if vs and rng.random() < stale_read and len(vs) > 1:
                v, u = vs[int(rng.integers(0, len(vs) - 1))]
            else:
                v, u = vs[-1] if vs else (None, None)
            body = (f":f :read :process {p} :value {'nil' if v is None else v} "
                    f":uid {'nil' if u is None else u}")
        elif op == 1:
            inv = f"{{:type :invoke :f :write :value {new} :process {p}{kk} :uid {uid} :time {inv_t}}}"
            body = f":f :write :process {p} :value {new} :uid {uid}"
            if ok:
                vs.append((new, uid))
        else:
            if vs and len(vs) > 1 and rng.random() < lost_update and vs[-2][0] != vs[-1][0]:
                cur = vs[-2][0]  # matched an older version: a lost update
                lost += ok
            elif vs:
                cur = vs[-1][0]
            else:
                cur, ok = int(rng.integers(0, 5)), False  # empty register: the update hits no row
            inv = (f"{{:type :invoke :f :cas :value [{cur} {new}] :process {p}{kk} :uid {uid} "
                   f":time {inv_t}}}")
            body = f":f :cas :process {p} :value [{cur} {new}] :uid {uid}"
            if ok:
                vs.append((new, uid))
        kind = ":ok" if ok else ":fail"
        lines.append((inv_t, len(lines), inv))
        lines.append((now, len(lines), f"{{:type {kind} {body}{kk} :time {now}}}"))
        busy[p] = now
    lines.sort()
    return "\n".join(l for _, _, l in lines) + "\n", lost


def adya_g2_edn(seed: int, n_keys: int = 500, anomaly: float = 0.05) -> Tuple[str, List[int]]:
    """adya.clj g2-gen's history (two concurrent inserts per key, one with an
    a-id and one with a b-id, globally unique ids): normally the first
    committer succeeds and the other fails serialization; with probability
    ``anomaly`` both complete :ok (G2).  Returns (EDN text, anomalous keys)."""
    rng = np.random.default_rng(seed)
    ids, t, lines, bad = 0, 1000, [], []
    for k in range(n_keys):
        pa, pb = 2 * (k % 8), 2 * (k % 8) + 1
        ids += 2
        a, b = ids - 1, ids
        both = rng.random() < anomaly
        first = int(rng.integers(0, 2))
        t0 = t
        lines.append(f"{{:type :invoke :f :insert :value [{k} [{a} nil]] :process {pa} :time {t0}}}")
        lines.append(f"{{:type :invoke :f :insert :value [{k} [nil {b}]] :process {pb} :time {t0 + 1}}}")
        for j, (p, val) in enumerate(((pa, f"[{k} [{a} nil]]"), (pb, f"[{k} [nil {b}]]"))):
            ok = both or j == first
            lines.append(f"{{:type {':ok' if ok else ':fail'} :f :insert :value {val} "
                         f":process {p} :time {t0 + 2 + j}}}")
        if both:
            bad.append(k)
        t += 10
    return "\n".join(lines) + "\n", bad


def txn_history_edn(seed: int, n_txns: int = 2000, n_procs: int = 8, n_keys: int = 50, fail: float = 0.05,
                    info: float = 0.03, dirty: float = 0.02, intermediate: float = 0.02) -> Tuple[str, dict]:
    """A multi-op txn history (``:f :txn``) of a serial execution with
    injected anomalies: ``fail`` of the txns complete :fail (their writes are
    not applied), ``info`` complete :info or never (applied half the time);
    a read returns with probability ``dirty`` a value a failed txn wrote and
    with probability ``intermediate`` a value its writer overwrote itself.
    Written values are unique.  Returns (EDN text, {"g1a": injected dirty
    reads of :ok txns, "g1b": injected intermediate reads of :ok txns})."""
    rng = np.random.default_rng(seed)
    latest: Dict[int, int] = {}
    dead: List[Tuple[int, int]] = []
    stale: List[Tuple[int, int]] = []
    lines: List[Tuple[int, int, str]] = []
    busy = np.zeros(n_procs, np.int64)
    now, nextv, inj = 1000, 1, {"g1a": 0, "g1b": 0}

    def fmt(ms, blank):
        return "[" + " ".join(f"[{f} {k} {'nil' if v is None or (blank and f == ':r') else v}]" for f, k, v in ms) + "]"

    for _ in range(n_txns):
        now += int(rng.integers(1, 50))
        p = int(rng.integers(0, n_procs))
        inv_t = max(int(busy[p]) + 1, now - int(rng.integers(0, 400)))
        u = rng.random()
        kind = ":fail" if u < fail else ":info" if u < fail + info else ":ok"
        applied = kind == ":ok" or (kind == ":info" and rng.random() < 0.5)
        ms, mine, a, b = [], {}, 0, 0
        for _ in range(int(rng.integers(1, 5))):
            k = int(rng.integers(0, n_keys))
            if rng.random() < 0.5:
                for q in range(2 if rng.random() < 0.15 else 1):
                    if k in mine:
                        stale.append((k, mine[k]))
                    mine[k] = nextv
                    ms.append((":w", k, nextv))
                    nextv += 1
            else:
                r = rng.random()
                if r < dirty and dead:
                    k, v = dead[int(rng.integers(0, len(dead)))]
                    a += 1
                elif r < dirty + intermediate and stale:
                    k, v = stale[int(rng.integers(0, len(stale)))]
                    b += 1
                else:
                    v = mine.get(k, latest.get(k))
                ms.append((":r", k, v))
        if applied:
            latest.update(mine)
        elif kind == ":fail":
            dead.extend(mine.items())
        if kind == ":ok":
            inj["g1a"] += a
            inj["g1b"] += b
        lines.append((inv_t, len(lines), f"{{:type :invoke :f :txn :value {fmt(ms, True)} :process {p} :time {inv_t}}}"))
        if kind != ":info" or rng.random() < 0.5:  # (the rest never complete)
            lines.append((now, len(lines), f"{{:type {kind} :f :txn :value {fmt(ms, kind != ':ok')} :process {p} "
                                           f":time {now}}}"))
            busy[p] = now
        else:
            busy[p] = now
            p_new = n_procs + len(lines)  # a crashed process never comes back
            lines[-1] = (inv_t, lines[-1][1], lines[-1][2].replace(f":process {p} ", f":process {p_new} "))
    lines.sort()
    return "\n".join(l for _, _, l in lines) + "\n", inj


def append_history_edn(seed: int, n_txns: int = 2000, n_procs: int = 24, n_keys: int = 50, fail: float = 0.05,
                       info: float = 0.03, lag: int = 200, dirty: float = 0.02, intermediate: float = 0.3,
                       dangling: float = 0.002, duplicate: float = 0.002, incompatible: float = 0.002,
                       cycles: bool = True) -> Tuple[str, dict]:
    """A list-append history (``:f :txn``, Elle's ``:append`` / ``:r``) of a
    serial execution with overlapping intervals: txn i takes effect at an
    instant inside [invoke, completion], and completes up to ``lag`` later, so
    completion order often differs from the order the appends were applied in.
    ``fail`` of the txns complete :fail (not applied), ``info`` complete :info
    or never (applied half the time).  Switches, each 0 / False for a clean
    history: ``dirty`` -- a failed txn's appends are applied all the same
    (G1a); ``intermediate`` -- of the txns that append twice to a key, the
    share whose state between the two is read by a concurrent txn (G1b);
    ``dangling`` / ``duplicate`` -- per append, an element nobody appended / a
    repeat of an element slips into the list; ``incompatible`` -- per read of
    two or more elements, the last two come back swapped; ``cycles`` -- one
    G0, G1c, G-single and G2 (write skew) on keys of their own at the end.
    With every switch off the history is strict serializable.  Returns (EDN
    text, the number of injections made per switch)."""
    rng = np.random.default_rng(seed)
    state: Dict[int, List[int]] = {}
    lines: List[Tuple[int, int, str]] = []
    busy = np.zeros(n_procs, np.int64)
    now, nextv, extra_proc = 1000, 1, n_procs
    inj = {"dirty": 0, "intermediate": 0, "dangling": 0, "duplicate": 0, "incompatible": 0, "cycles": 0}

    def fmt(ms, blank):
        def one(f, k, v):
            if f == ":append":
                return f"[:append {k} {v}]"
            return f"[:r {k} nil]" if blank else f"[:r {k} [{' '.join(str(x) for x in v)}]]"
        return "[" + " ".join(one(*m) for m in ms) + "]"

    def emit(p, inv_t, end_t, kind, ms):
        lines.append((inv_t, len(lines), f"{{:type :invoke :f :txn :value {fmt(ms, True)} :process {p} "
                                         f":time {inv_t}}}"))
        if end_t is not None:
            lines.append((end_t, len(lines), f"{{:type {kind} :f :txn :value {fmt(ms, kind != ':ok')} "
                                             f":process {p} :time {end_t}}}"))

    for _ in range(n_txns):
        now += int(rng.integers(1, 50))
        free = np.nonzero(busy < now)[0]
        if not len(free):
            now = int(busy.min()) + 1
            free = np.nonzero(busy < now)[0]
        p = int(free[int(rng.integers(0, len(free)))])
        inv_t = max(int(busy[p]) + 1, now - int(rng.integers(0, lag + 1)))
        end_t = now + int(rng.integers(0, lag + 1))
        u = rng.random()
        kind = ":fail" if u < fail else ":info" if u < fail + info else ":ok"
        applied = kind == ":ok" or (kind == ":info" and rng.random() < 0.5)
        if kind == ":fail" and rng.random() < dirty:
            applied = True
            inj["dirty"] += 1
        ms, work, between = [], {}, None

        def cur(k):
            if k not in work:
                work[k] = list(state.get(k, ()))
            return work[k]

        for _ in range(int(rng.integers(1, 5))):
            k = int(rng.integers(0, n_keys))
            if rng.random() < 0.5:
                twice = rng.random() < 0.15
                for q in range(2 if twice else 1):
                    lst = cur(k)
                    if rng.random() < dangling:
                        lst.append(10 ** 9 + nextv)  # nobody's element
                        inj["dangling"] += 1
                    if lst and rng.random() < duplicate:
                        lst.append(lst[int(rng.integers(0, len(lst)))])
                        inj["duplicate"] += 1
                    lst.append(nextv)
                    ms.append((":append", k, nextv))
                    nextv += 1
                    if twice and q == 0 and between is None and kind == ":ok" and rng.random() < intermediate:
                        between = (k, list(lst))
            else:
                v = list(cur(k))
                if len(v) >= 2 and rng.random() < incompatible:
                    v[-1], v[-2] = v[-2], v[-1]
                    inj["incompatible"] += 1
                ms.append((":r", k, v))
        if applied:
            state.update(work)
        if between is not None:  # a concurrent txn saw the list between the two appends
            emit(extra_proc, now - 1, now + 1, ":ok", [(":r", between[0], between[1])])
            extra_proc += 1
            inj["intermediate"] += 1
        if kind != ":info" or rng.random() < 0.5:
            emit(p, inv_t, end_t, kind, ms)
            busy[p] = end_t
        else:  # never completes: a crashed process does not come back
            emit(extra_proc, inv_t, None, kind, ms)
            extra_proc += 1
    if cycles:
        t0 = max([now] + [t for t, _, _ in lines]) + 1000
        k, v = 10 ** 6, nextv
        gadgets = [
            # G0: the version orders of two keys disagree
            [[(":append", k, v), (":append", k + 1, v + 1)], [(":append", k, v + 2), (":append", k + 1, v + 3)],
             [(":r", k, [v, v + 2]), (":r", k + 1, [v + 3, v + 1])]],
            # G1c: each read the other's append
            [[(":append", k + 2, v + 4), (":r", k + 3, [v + 5])], [(":append", k + 3, v + 5), (":r", k + 2, [v + 4])]],
            # G-single: one of the first txn's two appends seen, the other missed
            [[(":append", k + 4, v + 6), (":append", k + 5, v + 7)], [(":r", k + 4, [v + 6]), (":r", k + 5, [])],
             [(":r", k + 5, [v + 7])]],
            # G2: write skew
            [[(":r", k + 6, []), (":r", k + 7, []), (":append", k + 6, v + 8)],
             [(":r", k + 6, []), (":r", k + 7, []), (":append", k + 7, v + 9)],
             [(":r", k + 6, [v + 8]), (":r", k + 7, [v + 9])]],
        ]
        for g in gadgets:
            for ms in g:
                emit(extra_proc, t0, t0 + 10, ":ok", ms)
                extra_proc += 1
            t0 += 100
            inj["cycles"] += 1
    lines.sort()
    return "\n".join(l for _, _, l in lines) + "\n", inj


def dirty_reads_edn(seed: int, n_ops: int = 600, n_rows: int = 4, fail: float = 0.2,
                    dirty: float = 0.05) -> Tuple[str, List[List[int]]]:
    """The dirty-reads workload's history (core.clj:320-353) of a serial
    execution: writes of a fresh x to every row, ``fail`` of them :fail;
    reads return the rows' x (nothing before the first write: a short, empty
    read; sometimes a short read of a prefix).  With probability ``dirty`` a
    read shows a failed write's x in one row.  Returns (EDN text, the values
    of the dirty reads in order)."""
    rng = np.random.default_rng(seed)
    lines, injected, dead = [], [], []
    cur, x, t = None, 0, 1000
    for _ in range(n_ops):
        p = int(rng.integers(0, 5))
        t += 10
        if rng.random() < 0.5:
            x += 1
            ok = rng.random() >= fail
            lines.append(f"{{:type :invoke :f :write :value {x} :process {p} :time {t}}}")
            lines.append(f"{{:type {':ok' if ok else ':fail'} :f :write :value {x} :process {p} :time {t + 5}}}")
            if ok:
                cur = x
            else:
                dead.append(x)
        else:
            vals = [] if cur is None else [cur] * n_rows
            if vals and rng.random() < 0.2:
                vals = vals[: int(rng.integers(1, n_rows))]  # a short read
            if vals and dead and rng.random() < dirty:
                vals[int(rng.integers(0, len(vals)))] = dead[int(rng.integers(0, len(dead)))]
                injected.append(list(vals))
            lines.append(f"{{:type :invoke :f :read :value nil :process {p} :time {t}}}")
            lines.append(f"{{:type :ok :f :read :value [{' '.join(map(str, vals))}] :process {p} :time {t + 5}}}")
    return "\n".join(lines) + "\n", injected


def cas_register_history_edn(seed: int, n_ops: int = 1000, n_procs: int = 5, n_keys: int = 1, n_values: int = 5,
                             fail: float = 0.05, info: float = 0.02, stale: float = 0.0,
                             max_open: Optional[int] = None, independent: bool = False) -> Tuple[str, dict]:
    """A knossos-form history of the reference's register workload (core.clj:
    567-613: read / write / cas of ``rand-int n_values`` values, no ``:uid``)
    over one linearizable register per key, with overlapping ops: every op is
    invoked, takes effect at some later line and completes at a later one
    still, while other processes do the same.  ``fail`` of the ops complete
    ``:fail`` without an effect, as does a cas whose ``cur`` is not the
    register's value when it takes effect.  ``info`` of the writes and cas
    complete ``:info`` -- about half of them took effect -- and their process
    retires (its next op runs as process + n_procs, as Jepsen does); at most
    ``max_open`` of them per key when given.  With probability ``stale`` a read
    returns a value the register held before an overwrite that was already
    acknowledged when the read was invoked -- not linearizable unless an
    overlapping or open op may have written it back.  ``n_keys`` > 1: ``:key k``, or ``[k v]``
    values with ``independent``.  Returns (EDN text, {"stale": the completion
    lines of the injected reads, "info": ..., "info_effective": ...})."""
    rng = np.random.default_rng(seed)
    state: Dict[int, Optional[int]] = {k: None for k in range(n_keys)}
    acked: Dict[int, List[Optional[int]]] = {k: [] for k in range(n_keys)}  # values overwritten, the overwrite acknowledged
    opened = {k: 0 for k in range(n_keys)}
    procs = list(range(n_procs))
    busy: Dict[int, dict] = {}
    lines: List[str] = []
    inj = {"stale": [], "info": 0, "info_effective": 0}

    def fmt(k, v):
        body = "nil" if v is None else f"[{v[0]} {v[1]}]" if isinstance(v, tuple) else str(v)
        return (f":value [{k} {body}]" if independent else f":value {body}") + \
            (f" :key {k}" if n_keys > 1 and not independent else "")

    started = 0
    while started < n_ops or busy:
        idle = [i for i in range(n_procs) if i not in busy]
        if started < n_ops and idle and (not busy or rng.random() < 0.5):
            i = idle[int(rng.integers(0, len(idle)))]
            k = int(rng.integers(0, n_keys))
            f = (":read", ":write", ":cas")[int(rng.integers(0, 3))]
            v = None if f == ":read" else int(rng.integers(0, n_values))
            if f == ":cas":
                v = (int(rng.integers(0, n_values)), v)
            o = {"k": k, "f": f, "v": v, "phase": 0, "fate": ":ok", "old": list(acked[k])}
            r = rng.random()
            if r < fail:
                o["fate"] = ":fail"
            elif f != ":read" and r < fail + info and (max_open is None or opened[k] < max_open):
                o["fate"] = ":info"
                opened[k] += 1
            busy[i] = o
            started += 1
            lines.append(f"{{:type :invoke :f {f} {fmt(k, v)} :process {procs[i]} :time {len(lines)}}}")
            continue
        i = list(busy)[int(rng.integers(0, len(busy)))]
        o = busy[i]
        k, f, v = o["k"], o["f"], o["v"]
        if o["phase"] == 0:  # takes effect
            o["phase"] = 1
            if o["fate"] == ":fail" or (o["fate"] == ":info" and rng.random() < 0.5):
                continue
            if f == ":read":
                o["v"] = state[k]
                older = [x for x in o["old"] if x is not None and x != state[k]]  # (a nil read is a wildcard)
                if older and rng.random() < stale:
                    o["v"] = older[int(rng.integers(0, len(older)))]
                    o["stale"] = True
            elif f == ":write" or state[k] == v[0]:
                o["prev"], o["applied"] = state[k], True
                state[k] = v if f == ":write" else v[1]
            else:
                o["fate"] = ":fail" if o["fate"] == ":ok" else o["fate"]
            continue
        del busy[i]
        if o.get("stale"):
            inj["stale"].append(len(lines))
        if o["fate"] == ":info":
            inj["info"] += 1
            inj["info_effective"] += bool(o.get("applied"))
        elif o.get("applied"):
            acked[k].append(o["prev"])
        lines.append(f"{{:type {o['fate']} :f {f} {fmt(k, o['v'])} :process {procs[i]} :time {len(lines)}}}")
        if o["fate"] == ":info":
            procs[i] += n_procs
    return "\n".join(lines) + "\n", inj


def _interleave(rng, n_procs: int, n_items: int, invoke, complete) -> List[str]:
    """Lines of n_items ops run by n_procs processes, one op in flight per
    process: ``invoke(i, p)`` / ``complete(i, p)`` give an op's two lines."""
    lines, pending, nxt = [], {}, 0
    while nxt < n_items or pending:
        p = int(rng.integers(0, n_procs))
        if p in pending:
            lines.append(complete(pending.pop(p), p))
        elif nxt < n_items:
            lines.append(invoke(nxt, p))
            pending[p] = nxt
            nxt += 1
    return lines


def set_history_edn(seed: int, n_adds: int = 1000, n_procs: int = 5, lose: int = 0, phantom: int = 0,
                    info_frac: float = 0.0) -> Tuple[str, dict]:
    """A sets-test history (core.clj:252-272): adds of 0 .. n_adds - 1 by
    n_procs processes, each ``:ok``, ``:fail`` (3 %, not in the set) or, with
    probability ``info_frac``, ``:info`` (in the set or not, a coin each), then
    one final read.  ``lose`` acknowledged adds are missing from the read,
    ``phantom`` values nobody added are in it.  Returns (EDN text, the
    injected ``lost`` / ``unexpected`` / ``recovered`` values, sorted, and
    ``ok``, the attempted values the read holds)."""
    rng = np.random.default_rng(seed)
    kind = np.where(rng.random(n_adds) < info_frac, 2, np.where(rng.random(n_adds) < 0.03, 1, 0))
    names = (":ok", ":fail", ":info")
    lines = _interleave(rng, n_procs, n_adds,
                        lambda i, p: f"{{:type :invoke, :f :add, :value {i}, :process {p}}}",
                        lambda i, p: f"{{:type {names[kind[i]]}, :f :add, :value {i}, :process {p}}}")
    acked = np.flatnonzero(kind == 0)
    lost = np.sort(rng.choice(acked, size=min(lose, len(acked)), replace=False)) if lose else np.zeros(0, np.int64)
    infos = np.flatnonzero(kind == 2)
    recovered = infos[rng.random(len(infos)) < 0.5]
    unexpected = n_adds + 100 + 2 * np.arange(phantom)
    final = np.sort(np.concatenate([np.setdiff1d(acked, lost), recovered, unexpected])).astype(np.int64)
    lines.append("{:type :invoke, :f :read, :value nil, :process 0}")
    lines.append("{:type :ok, :f :read, :value #{" + " ".join(str(int(v)) for v in final) + "}, :process 0}")
    inj = {"lost": [int(v) for v in lost], "unexpected": [int(v) for v in unexpected],
           "recovered": [int(v) for v in recovered], "ok": [int(v) for v in final if v < n_adds]}
    return "\n".join(lines) + "\n", inj


def queue_history_edn(seed: int, n_enqueues: int = 1000, n_procs: int = 5, n_values: int = 64, lose: int = 0,
                      duplicate: int = 0, unexpected: int = 0, info_frac: float = 0.0) -> Tuple[str, dict]:
    """A total-queue history: n_enqueues enqueues of values below n_values
    (so values repeat), then a drain.  Values of the upper half may complete
    ``:info`` (probability ``info_frac``; dequeued or not, a coin each); the
    injections touch the lower half only, one value each, so that they add up
    exactly: ``lose`` acknowledged elements never dequeued, ``duplicate``
    extra dequeues of a value every enqueue of which was acknowledged and
    dequeued, ``unexpected`` dequeues of values nobody enqueued.  Returns
    (EDN text, the injected ``lost`` / ``duplicated`` / ``unexpected`` /
    ``recovered`` multisets as sorted (value, count) lists)."""
    rng = np.random.default_rng(seed)
    half = max(n_values // 2, 1)
    vals = rng.integers(0, n_values, n_enqueues)
    info = (vals >= half) & (rng.random(n_enqueues) < info_frac)
    lines = _interleave(rng, n_procs, n_enqueues,
                        lambda i, p: f"{{:type :invoke, :f :enqueue, :value {vals[i]}, :process {p}}}",
                        lambda i, p: (f"{{:type {':info' if info[i] else ':ok'}, :f :enqueue, :value {vals[i]}, "
                                      f":process {p}}}"))
    out = list(vals[~info])
    low = np.unique(vals[vals < half])
    picks = rng.permutation(low)[:min(lose + duplicate, len(low))]
    lost, dup = {}, {}
    for v in picks[:lose]:
        lost[int(v)] = int(rng.integers(1, int((vals == v).sum()) + 1))
        for _ in range(lost[int(v)]):
            out.remove(v)
    for v in picks[lose:]:
        dup[int(v)] = int(rng.integers(1, 4))
        out += [v] * dup[int(v)]
    rec = {}
    for v in vals[info][rng.random(int(info.sum())) < 0.5]:
        rec[int(v)] = rec.get(int(v), 0) + 1
        out.append(v)
    unx = {}
    for k in range(unexpected):
        unx[n_values + 100 + 3 * k] = 1 + k % 2
        out += [n_values + 100 + 3 * k] * (1 + k % 2)
    out = [int(v) for v in rng.permutation(np.array(out, np.int64))]
    lines += _interleave(rng, n_procs, len(out),
                         lambda i, p: f"{{:type :invoke, :f :dequeue, :value nil, :process {p}}}",
                         lambda i, p: f"{{:type :ok, :f :dequeue, :value {out[i]}, :process {p}}}")
    inj = {"lost": sorted(lost.items()), "duplicated": sorted(dup.items()), "unexpected": sorted(unx.items()),
           "recovered": sorted(rec.items())}
    return "\n".join(lines) + "\n", inj


def bank_history_edn(seed: int, n: int = 5, start: int = 10, n_ops: int = 500, n_procs: int = 5,
                     skew_reads: int = 0, short_reads: int = 0) -> Tuple[str, dict]:
    """A bank-test history (core.clj:71-150, :297-318): n accounts of
    ``start`` each, n_ops ops, half reads and half transfers, executed in
    order (a transfer that would go negative completes ``:fail``).
    ``skew_reads`` reads are snapshots taken between the two updates of a
    transfer of at least 1 -- they miss its credit; ``short_reads`` reads lack
    their last balance.  Returns (EDN text, ``skewed``: [(read, amount)] and
    ``short``: [read], reads numbered among the ``:ok`` reads in history
    order)."""
    rng = np.random.default_rng(seed)
    bal = [start] * n
    is_read = rng.random(n_ops) < 0.5
    reads = np.flatnonzero(is_read)
    marked = rng.permutation(reads)[:skew_reads + short_reads]
    skew_at, short_at = set(marked[:skew_reads].tolist()), set(marked[skew_reads:].tolist())
    lines, skewed, short, nread = [], [], [], 0
    for i in range(n_ops):
        p = int(rng.integers(0, n_procs))
        if is_read[i]:
            lines.append(f"{{:type :invoke, :f :read, :process {p}}}")
            snap = list(bal)
            if i in skew_at:  # a transfer by another process, seen half done
                src = int(rng.choice([a for a in range(n) if bal[a] >= 1]))
                dst = (src + 1 + int(rng.integers(0, max(n - 1, 1)))) % n
                amount = int(rng.integers(1, min(bal[src], 4) + 1))
                q = (p + 1) % max(n_procs, 2)
                val = f"{{:from {src}, :to {dst}, :amount {amount}}}"
                lines.insert(len(lines) - 1, f"{{:type :invoke, :f :transfer, :value {val}, :process {q}}}")
                snap[src] -= amount
                bal[src] -= amount
                bal[dst] += amount
                skewed.append((nread, amount))
            elif i in short_at:
                snap = snap[:-1]
                short.append(nread)
            lines.append(f"{{:type :ok, :f :read, :value [{' '.join(map(str, snap))}], :process {p}}}")
            if i in skew_at:
                lines.append(f"{{:type :ok, :f :transfer, :value {val}, :process {q}}}")
            nread += 1
            continue
        src, dst, amount = int(rng.integers(0, n)), int(rng.integers(0, n)), int(rng.integers(0, 5))
        val = f"{{:from {src}, :to {dst}, :amount {amount}}}"
        lines.append(f"{{:type :invoke, :f :transfer, :value {val}, :process {p}}}")
        if bal[src] - amount < 0:
            lines.append(f"{{:type :fail, :f :transfer, :value [:negative {src} {bal[src] - amount}], :process {p}}}")
        else:
            bal[src] -= amount
            bal[dst] += amount
            lines.append(f"{{:type :ok, :f :transfer, :value {val}, :process {p}}}")
    return "\n".join(lines) + "\n", {"skewed": skewed, "short": short}


def _kv(n_keys: int, k: int, v) -> str:
    v = "nil" if v is None else str(v)
    return f"[{k} {v}]" if n_keys else v


def counter_history_edn(seed: int, n_ops: int = 400, n_procs: int = 5, n_keys: int = 0, fail: float = 0.05,
                        info: float = 0.05, bad_reads: int = 0, malformed: int = 0) -> Tuple[str, dict]:
    """A counter history: adds of 1 .. 5 and reads by n_procs processes, one
    op in flight per process, executed against a real counter at completion
    (an ``:ok`` add counts, a ``:fail`` one does not, an ``:info`` one may, and
    retires its process).  ``n_keys`` > 0: that many independent counters, the
    values ``[k v]`` tuples.  ``bad_reads`` reads return one more than every
    add attempted so far could give; ``malformed`` ops complete twice.
    Returns (EDN text, {"bad": the keys with such a read, "malformed": the
    keys with such an op}; key 0 stands for the single counter)."""
    rng = np.random.default_rng(seed)
    nk = max(n_keys, 1)
    is_add = rng.random(n_ops) < 0.5
    amount = rng.integers(1, 6, n_ops)
    okey = rng.integers(0, nk, n_ops)
    fate = rng.choice(3, n_ops, p=[1 - fail - info, fail, info])  # ok, fail, info
    reads = np.flatnonzero(~is_add & (fate == 0))
    bad_at = set(rng.choice(reads, min(bad_reads, len(reads)), replace=False).tolist()) if bad_reads else set()
    twice = set(rng.choice(n_ops, min(malformed, n_ops), replace=False).tolist()) if malformed else set()
    actual, upper, gen = [0] * nk, [0] * nk, [0] * n_procs
    inj = {"bad": set(), "malformed": set()}

    def pid(p):
        return p + n_procs * gen[p]

    def invoke(i, p):
        k = int(okey[i])
        if is_add[i]:
            upper[k] += int(amount[i])
            return f"{{:type :invoke, :f :add, :value {_kv(n_keys, k, int(amount[i]))}, :process {pid(p)}}}"
        return f"{{:type :invoke, :f :read, :value {_kv(n_keys, k, None)}, :process {pid(p)}}}"

    def complete(i, p):
        k, t, me = int(okey[i]), (":ok", ":fail", ":info")[fate[i]], pid(p)
        if is_add[i]:
            if fate[i] == 0 or (fate[i] == 2 and rng.random() < 0.5):
                actual[k] += int(amount[i])
            v = int(amount[i])
        else:
            v = None if fate[i] else upper[k] + 1 if i in bad_at else actual[k]
            if i in bad_at:
                inj["bad"].add(k)
        if fate[i] == 2:
            gen[p] += 1
        line = f"{{:type {t}, :f {':add' if is_add[i] else ':read'}, :value {_kv(n_keys, k, v)}, :process {me}}}"
        if i in twice and fate[i] != 2:
            inj["malformed"].add(k)
            return line + "\n" + line
        return line

    lines = _interleave(rng, n_procs, n_ops, invoke, complete)
    return "\n".join(lines) + "\n", {k: sorted(v) for k, v in inj.items()}


def fifo_queue_history_edn(seed: int, n_ops: int = 400, n_procs: int = 5, n_keys: int = 0, swap: int = 0,
                           phantom: int = 0, fail_enq: float = 0.05) -> Tuple[str, dict]:
    """A queue history that both of checker/queue's models accept: enqueues of
    distinct values (in the queue from their invocation, ``fail_enq`` of them
    completing ``:fail``, as the checker counts them) and dequeues that take
    the head of a real FIFO queue at completion (``:fail`` on an empty one).
    ``n_keys`` > 0: independent queues, ``[k v]`` values.  ``swap`` dequeues
    take the second element instead (illegal for fifo-queue only),
    ``phantom`` dequeues return a value nobody enqueued (illegal for both).
    Returns (EDN text, {"swapped": keys, "phantom": keys})."""
    rng = np.random.default_rng(seed)
    nk = max(n_keys, 1)
    is_enq = rng.random(n_ops) < 0.55
    okey = rng.integers(0, nk, n_ops)
    failed = rng.random(n_ops) < fail_enq
    deqs = np.flatnonzero(~is_enq)
    picks = rng.permutation(deqs)[:swap + phantom].tolist()
    swap_at, phantom_at = set(picks[:swap]), set(picks[swap:])
    queues = [collections.deque() for _ in range(nk)]
    inj = {"swapped": set(), "phantom": set()}

    def invoke(i, p):
        k = int(okey[i])
        if is_enq[i]:
            queues[k].append(i)
            return f"{{:type :invoke, :f :enqueue, :value {_kv(n_keys, k, i)}, :process {p}}}"
        return f"{{:type :invoke, :f :dequeue, :value {_kv(n_keys, k, None)}, :process {p}}}"

    def complete(i, p):
        k, q = int(okey[i]), queues[int(okey[i])]
        if is_enq[i]:
            t = ":fail" if failed[i] else ":ok"
            return f"{{:type {t}, :f :enqueue, :value {_kv(n_keys, k, i)}, :process {p}}}"
        if i in phantom_at:
            inj["phantom"].add(k)
            v = 10 ** 6 + i
        elif not q:
            return f"{{:type :fail, :f :dequeue, :value {_kv(n_keys, k, None)}, :process {p}}}"
        elif i in swap_at and len(q) >= 2:
            inj["swapped"].add(k)
            v = q[1]
            del q[1]
        else:
            v = q.popleft()
        return f"{{:type :ok, :f :dequeue, :value {_kv(n_keys, k, v)}, :process {p}}}"

    lines = _interleave(rng, n_procs, n_ops, invoke, complete)
    return "\n".join(lines) + "\n", {k: sorted(v) for k, v in inj.items()}
