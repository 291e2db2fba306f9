"""CPU model of the perf checker: a plain Python restatement of the
reference's jepsen/checker/perf.clj and of util/history->latencies and
util/nemesis-intervals (jepsen/util.clj), written from their text, line-cited.
The reference's Clojure cannot be run here (there is no JVM), so this is a
restatement, as tally_model.py is -- kept as close to the text as Python
allows: a sequential reduce with a dict, ``sorted``, float arithmetic in the
reference's order, no numpy tricks.  hsc_perf_check (include/hip_serial.h) and
jepsen.perf_report are compared with it.

Two layers:
  * ``graphs(history)``: the data sets exactly as the three graph functions
    and ``rate`` build them from a history of op dicts (keys "type", "f",
    "process", "time" with the EDN spellings ":invoke", 3, ":nemesis" ...);
  * ``perf(...)``: the same computation over the interned columns, in the
    shape of ``Validator.perf_check``'s dict (cells instead of maps).
Unpaired invokes: the reference throws on them (latency-point divides nil);
both layers leave them out, as the entry does."""
import decimal
import math

INVOKE, OK, FAIL, INFO = 0, 1, 2, 3
TYPES = (":invoke", ":ok", ":fail", ":info")
GRAPH_TYPES = (":ok", ":info", ":fail")  # perf.clj:158-160
ALL = ":jepsen.checker.perf/all"         # ::all
CELL_CAP = 65536                         # HSC_PERF_CELL_CAP
QS = (0.5, 0.95, 0.99, 1)                # perf.clj:251
INT64_MAX = (1 << 63) - 1


# ---- util.clj -----------------------------------------------------------------
def nanos_to_secs(ns):
    return ns / 1e9  # util.clj:220 (/ nanos 1e9)


def nanos_to_ms(ns):
    """(double (/ nanos 1000000)), util.clj:216 under perf.clj:134: a ratio made
    a double.  Ratio.doubleValue goes through 16 decimal digits (half even)."""
    if ns % 1000000 == 0:
        return float(ns // 1000000)  # (a long, not a ratio)
    ctx = decimal.Context(prec=16, rounding=decimal.ROUND_HALF_EVEN)
    return float(ctx.divide(decimal.Decimal(ns), decimal.Decimal(1000000)))


def history_latencies(history):
    """util/history->latencies (util.clj:553-587): copies of the ops, every
    completed invoke with "latency" and "completion" (the completion's index
    here), every completion that found an invoke with "latency"."""
    out, invokes = [], {}
    for op in history:
        op = dict(op)
        if op["type"] == ":invoke":  # :565-569
            out.append(op)
            invokes[op["process"]] = len(out) - 1
        elif op["process"] in invokes:  # :571-581
            i = invokes.pop(op["process"])
            lat = op["time"] - out[i]["time"]
            op["latency"] = lat
            out.append(op)
            out[i]["latency"], out[i]["completion"] = lat, len(out) - 1
        else:  # :583-584
            out.append(op)
    return out


def util_nemesis_intervals(history):
    """util/nemesis-intervals (util.clj:589-606): [start op, stop op or None]."""
    pairs, starts = [], []
    for op in history:
        if op["process"] != ":nemesis":
            continue
        if op["f"] == ":start":
            starts.append(op)
        elif op["f"] == ":stop":  # (peek / pop of an empty queue: nil / the empty queue)
            pairs.append((starts[0] if starts else None, op))
            starts = starts[1:]
    return pairs + [(s, None) for s in starts]


# ---- perf.clj -----------------------------------------------------------------
def bucket_scale(dt, b):
    return int(b) * dt + dt / 2  # :15-19


def bucket_time(dt, t):
    return bucket_scale(dt, t / dt)  # :21-25


def bucket_index(dt, t_ns):
    return int(nanos_to_secs(t_ns) / dt)  # the long of :19 under :25, of a time in ns


def buckets(dt, tmax):
    out, b = [], 0  # :27-34
    while tmax >= bucket_scale(dt, b):
        out.append(bucket_scale(dt, b))
        b += 1
    return out


def quantiles(qs, points):
    s = sorted(points)  # :45-55
    if not s:
        return None
    n = len(s)
    return {q: s[min(n - 1, int(math.floor(n * q)))] for q in qs}


def latencies_quantiles(dt, qs, points):
    by = {}  # :57-79; bucket-points :36-43
    for t, lat in points:
        by.setdefault(bucket_time(dt, t), []).append(lat)
    bs = [(t, quantiles(qs, by[t])) for t in sorted(by)]
    return {q: [(t, m[q]) for t, m in bs] for q in qs}


def latency_point(op):
    return (float(nanos_to_secs(op["time"])), nanos_to_ms(op["latency"]))  # :129-134


def nemesis_intervals(history):
    times = [op["time"] for op in history if op.get("time") is not None]  # :168-187 (0 is truthy there)
    final = float(nanos_to_secs(times[-1])) if times else None
    return [(float(nanos_to_secs(a["time"])), float(nanos_to_secs(b["time"])) if b else final)
            for a, b in util_nemesis_intervals(history) if a]


def rate(history):
    m = {}  # :113-127
    for op in history:
        if op["type"] == ":invoke":
            continue
        for a, b in ((op["f"], op["type"]), (op["f"], ALL), (ALL, op["type"]), (ALL, ALL)):
            m.setdefault(a, {})
            m[a][b] = m[a].get(b, 0) + 1
    return m


def graphs(history, qs=QS, q_dt=30, r_dt=10):
    """{"latency_raw", "latency_quantiles", "rate", "counts",
    "nemesis_intervals"}: the data sets of point-graph! (:220-244),
    quantiles-graph! (:246-282), rate-graph! (:293-331), rate and
    nemesis-intervals, over the paired invokes."""
    h = history_latencies(history)
    inv = [op for op in h if op["type"] == ":invoke"]
    by_f = {}
    for op in inv:  # invokes-by-f :89-94
        by_f.setdefault(op["f"], []).append(op)
    paired = {f: [op for op in ops if "completion" in op] for f, ops in by_f.items()}
    raw = {f: {t: [latency_point(op) for op in ops if h[op["completion"]]["type"] == t] for t in GRAPH_TYPES}
           for f, ops in paired.items()}  # invokes-by-f-type :81-102
    quant = {f: latencies_quantiles(q_dt, qs, [latency_point(op) for op in ops]) for f, ops in paired.items()}
    td = float(1 / r_dt)  # :297
    t_max = nanos_to_secs(max([0] + [op["time"] for op in history]))  # :298
    data = {}
    for op in history:  # :299-311
        if op["type"] == ":invoke" or type(op["process"]) is not int:
            continue
        cell = data.setdefault(op["f"], {}).setdefault(op["type"], {})
        k = bucket_time(r_dt, nanos_to_secs(op["time"]))
        cell[k] = td + cell.get(k, 0)
    mids = buckets(r_dt, t_max)
    rates = {f: {t: [(m, d.get(t, {}).get(m, 0)) for m in mids] for t in GRAPH_TYPES} for f, d in data.items()}
    return {"latency_raw": raw, "latency_quantiles": quant, "rate": rates, "counts": rate(history),
            "nemesis_intervals": nemesis_intervals(history)}


# ---- the entry's shape --------------------------------------------------------
def perf(type, f, process, client, time, nf, qs=QS, q_dt=30, r_dt=10, arrays=False, cap=CELL_CAP):
    """What ``Validator.perf_check`` returns for these columns (all but ``ms``,
    ``phase_ms`` and ``sort_packed``), lists for arrays."""
    n = len(type)
    comp, inv, lat = [-1] * n, [-1] * n, [0] * n
    open_ = {}
    for i in range(n):  # history->latencies
        p = int(process[i])
        if type[i] == INVOKE:
            open_[p] = i
        elif p in open_:
            j = open_.pop(p)
            comp[j], inv[i] = i, j
            lat[j] = int(time[i]) - int(time[j])
    paired = [i for i in range(n) if comp[i] >= 0]
    cells = {}
    for i in paired:
        cells.setdefault((int(f[i]), bucket_index(q_dt, int(time[i]))), []).append(lat[i])
    keys = sorted(cells)
    listed = keys[:cap]
    cell_lat = []
    for k in listed:
        s = sorted(cells[k])
        cell_lat.append([s[min(len(s) - 1, int(math.floor(len(s) * q)))] for q in qs])
    rcells, counts = {}, [[0] * 4 for _ in range(nf)]
    for i in range(n):
        if type[i] == INVOKE:
            continue
        counts[int(f[i])][int(type[i])] += 1
        if client[i]:
            k = (int(f[i]), int(type[i]), bucket_index(r_dt, int(time[i])))
            rcells[k] = rcells.get(k, 0) + 1
    rkeys = sorted(rcells)
    rl = rkeys[:cap]
    invokes = sum(1 for t in type if t == INVOKE)
    out = {"n": n, "invokes": invokes, "paired": len(paired), "unpaired": invokes - len(paired),
           "orphans": sum(1 for i in range(n) if type[i] != INVOKE and inv[i] < 0),
           "t_max": max([0] + [int(t) for t in time]), "cells": len(keys), "rate_cells": len(rkeys),
           "cells_listed": len(listed), "rate_listed": len(rl),
           "cell_f": [k[0] for k in listed], "cell_bucket": [k[1] for k in listed],
           "cell_count": [len(cells[k]) for k in listed], "cell_lat": cell_lat,
           "rate_f": [k[0] for k in rl], "rate_type": [k[1] for k in rl], "rate_bucket": [k[2] for k in rl],
           "rate_count": [rcells[k] for k in rl], "counts": counts,
           "qs": tuple(qs), "q_dt": q_dt, "r_dt": r_dt}
    if arrays:
        groups = [[] for _ in range(nf * 4)]
        for i in paired:  # invokes-by-f-type: history order inside a group
            groups[int(f[i]) * 4 + int(type[comp[i]])].append(i)
        off = [0]
        for g in groups:
            off.append(off[-1] + len(g))
        out.update(completion_of=comp, invoke_of=inv, latency=lat, raw_op=[i for g in groups for i in g], raw_off=off)
    return out


SCALARS = ("n", "invokes", "paired", "unpaired", "orphans", "t_max", "cells", "rate_cells", "cells_listed",
           "rate_listed")
ARRAYS = ("cell_f", "cell_bucket", "cell_count", "cell_lat", "rate_f", "rate_type", "rate_bucket", "rate_count",
          "counts")
OP_ARRAYS = ("completion_of", "invoke_of", "latency", "raw_op", "raw_off")


def _list(x):
    return x.tolist() if hasattr(x, "tolist") else [(_list(r) if isinstance(r, (list, tuple)) else r) for r in x]


def assert_same_perf(got, want):
    """Every field of the entry's dict against the model's, exactly."""
    for k in SCALARS:
        assert int(got[k]) == int(want[k]), (k, got[k], want[k])
    for k in ARRAYS + (OP_ARRAYS if "raw_op" in want else ()):
        g, w = _list(got[k]), _list(want[k])
        if k == "cell_lat" and not w:
            assert len(g) == 0, k
            continue
        assert g == w, (k, g[:8], w[:8])
    assert ("raw_op" in got) == ("raw_op" in want)


def history_of(type, f, process, client, time, fs=None, processes=None):
    """The columns as op dicts for ``graphs``: a client's process is its id (an
    int), any other ":p<id>" unless ``processes`` names it."""
    out = []
    for i in range(len(type)):
        p = int(process[i])
        name = processes[p] if processes is not None else (p if client[i] else f":p{p}")
        out.append({"type": TYPES[int(type[i])], "f": fs[int(f[i])] if fs is not None else int(f[i]), "process": name,
                    "time": int(time[i])})
    return out
