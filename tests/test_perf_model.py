"""CPU: the perf model (perf_model.py) against hand-worked answers, and the
pure Python half of the perf checker and of the composition in
comdb2_amd/jepsen.py -- perf_ops_from_edn, perf_report, with_times,
merge_valid, compose_edn -- against the model.  Also the window arithmetic:
where the reference's double expression agrees with integer division, and that
the model follows the doubles where it does not."""
import numpy as np
import pytest

import perf_model as PM
from comdb2_amd import jepsen as J

S = 10 ** 9


def op(type, f, process, time):
    return {"type": type, "f": f, "process": process, "time": time}


def edn(history):
    return "\n".join(f"{{:type {o['type']}, :f {o['f']}, :process {o['process']}, :time {o['time']}}}"
                     for o in history) + "\n"


HAND = [
    op(":invoke", ":read", 0, 1 * S), op(":invoke", ":write", 1, 2 * S), op(":ok", ":read", 0, 3 * S),
    op(":info", ":start", ":nemesis", 4 * S), op(":info", ":start", ":nemesis", 5 * S),
    op(":fail", ":write", 1, 12 * S), op(":invoke", ":read", 0, 31 * S), op(":invoke", ":read", 0, 32 * S),
    op(":info", ":read", 0, 36 * S), op(":ok", ":read", 0, 37 * S),
    op(":info", ":stop", ":nemesis", 38 * S), op(":info", ":stop", ":nemesis", 39 * S),
    op(":info", ":start", ":nemesis", 40 * S),
]


def test_model_hand_worked():
    h = PM.history_latencies(HAND)
    assert [(o.get("latency"), o.get("completion")) for o in h if o["type"] == ":invoke"] == \
        [(2 * S, 2), (10 * S, 5), (None, None), (4 * S, 8)]  # the invoke at 31 s was overwritten
    g = PM.graphs(HAND)
    assert g["latency_raw"] == {":read": {":ok": [(1.0, 2000.0)], ":info": [(32.0, 4000.0)], ":fail": []},
                                ":write": {":ok": [], ":info": [], ":fail": [(2.0, 10000.0)]}}
    assert g["latency_quantiles"][":read"][0.5] == [(15, 2000.0), (45, 4000.0)]
    assert g["latency_quantiles"][":write"][1] == [(15, 10000.0)]
    # t-max 40 s: midpoints 5 .. 35; the completions at 36 and 37 s lie in the window of midpoint 35
    assert g["rate"][":read"][":ok"] == [(5, 0.1), (15, 0), (25, 0), (35, 0.1)]
    assert g["rate"][":read"][":info"] == [(5, 0), (15, 0), (25, 0), (35, 0.1)]
    assert g["rate"][":write"][":fail"] == [(5, 0), (15, 0.1), (25, 0), (35, 0)]
    assert ":start" not in g["rate"]  # the nemesis is not graphed
    assert g["counts"][PM.ALL] == {":ok": 2, ":fail": 1, ":info": 6, PM.ALL: 9}
    assert g["counts"][":start"] == {":info": 3, PM.ALL: 3}
    # start start stop stop pairs first with third, second with fourth; the open start ends at the last time
    assert g["nemesis_intervals"] == [(4.0, 38.0), (5.0, 39.0), (40.0, 40.0)]


def test_model_quantile_index_and_rate_sum():
    assert PM.quantiles((0, 0.5, 0.95, 0.999, 1), list(range(20, 0, -1))) == {0: 1, 0.5: 11, 0.95: 20, 0.999: 20, 1: 20}
    assert PM.quantiles((0.5,), []) is None
    # 1 / dt added six times is not 6 / dt
    h = [op(":ok", ":r", 0, k) for k in range(5)]
    six = 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1
    assert PM.graphs(h + [op(":ok", ":r", 0, 6 * S)])["rate"][":r"][":ok"] == [(5, six)]
    assert six != 6 * 0.1
    # the t-max rule: the only completion of the last window lies past the last listed midpoint
    assert PM.graphs([op(":ok", ":r", 0, 1 * S), op(":ok", ":r", 0, 12 * S)])["rate"][":r"][":ok"] == [(5, 0.1)]


def test_nanos_to_ms_through_sixteen_digits():
    for ns in (0, 1, -1, 1234567, 10 ** 16 - 1, -(10 ** 16) + 1, 5 * 10 ** 17, PM.INT64_MAX, -PM.INT64_MAX):
        assert PM.nanos_to_ms(ns) == J.nanos_to_ms(ns), ns
    assert PM.nanos_to_ms(1234567) == 1.234567
    assert PM.nanos_to_ms(PM.INT64_MAX) == float("9223372036854.776")  # 16 digits, then the nearest double


def columns(history):
    ops = J.perf_ops_from_edn(edn(history))
    return ops, (ops.type, ops.f, ops.process, ops.client, ops.time, len(ops.fs))


def test_perf_ops_from_edn():
    ops, _ = columns(HAND)
    assert ops.fs == [":read", ":start", ":stop", ":write"]  # util/polysort: keywords by name
    assert ops.processes == [0, 1, ":nemesis"]
    assert ops.type.tolist() == [0, 0, 1, 3, 3, 2, 0, 0, 3, 1, 3, 3, 3]
    assert ops.client.tolist() == [1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0]
    assert ops.nemesis == [(":start", 4 * S), (":start", 5 * S), (":stop", 38 * S), (":stop", 39 * S), (":start", 40 * S)]
    assert ops.time.dtype == np.int64 and ops.f.dtype == np.uint32 and ops.type.dtype == np.uint8
    # an integer and a keyword process are different processes; nil and non-keyword fs order as polysort does
    mixed = J.perf_ops_from_edn("{:type :ok, :f 3, :process 1, :time 5}\n{:type :ok, :f nil, :process :a, :time 6}\n"
                                "{:type :ok, :f :x, :process nil, :time 7}\n")
    assert mixed.fs == [None, ":x", 3] and mixed.processes == [1, ":a", None] and mixed.client.tolist() == [1, 0, 0]
    for bad in ("{:type :ok, :f :x, :process 1}", "{:type :ok, :f :x, :process 1, :time nil}",
                "{:type :ok, :f :x, :process 1, :time -1}", "{:type :done, :f :x, :process 1, :time 1}"):
        with pytest.raises(ValueError):
            J.perf_ops_from_edn(bad)
    assert len(J.perf_ops_from_edn("").type) == 0


def same_graphs(rep, g):
    for k in ("latency_quantiles", "rate", "counts", "nemesis_intervals"):
        assert rep[k] == g[k], k
    if "latency_raw" in rep:
        assert rep["latency_raw"] == g["latency_raw"]


def test_perf_report_on_a_hand_made_res():
    ops, _ = columns(HAND)
    res = {"n": 13, "invokes": 4, "paired": 3, "unpaired": 1, "orphans": 6, "t_max": 40 * S, "cells": 3,
           "rate_cells": 4, "cells_listed": 3, "rate_listed": 4, "qs": (0.5, 1), "q_dt": 30, "r_dt": 10,
           "cell_f": np.array([0, 0, 3]), "cell_bucket": np.array([0, 1, 0]), "cell_count": np.array([1, 1, 1]),
           "cell_lat": np.array([[2 * S] * 2, [4 * S] * 2, [10 * S] * 2]),
           "rate_f": np.array([0, 0, 0, 3]), "rate_type": np.array([1, 1, 3, 2]),
           "rate_bucket": np.array([0, 3, 3, 1]), "rate_count": np.array([1, 1, 1, 1]),
           "counts": np.array([[0, 2, 0, 1], [0, 0, 0, 3], [0, 0, 0, 2], [0, 0, 1, 0]])}
    rep = J.perf_report(ops, res)
    g = PM.graphs(HAND, qs=(0.5, 1))
    same_graphs(rep, g)
    assert rep["valid"] is True and rep["truncated"] == [] and "latency_raw" not in rep and rep["perf"] is res
    assert (rep["unpaired"], rep["orphans"], rep["t_max"]) == (1, 6, 40 * S)
    res.update(cells=70000, rate_cells=70001)
    assert J.perf_report(ops, res)["truncated"] == ["latency_quantiles", "rate"]


def random_history(seed, n_ops=400, n_procs=5, n_f=3, nemesis=True, span=200 * S):
    """Ops of n_procs clients with every pairing shape -- double invokes, lone
    completions -- at sorted random times, nemesis ops among them."""
    rng = np.random.default_rng(seed)
    times = np.sort(rng.integers(0, span, n_ops))
    out, open_ = [], {}
    for t in times.tolist():
        u = rng.random()
        if nemesis and u < 0.03:
            out.append(op(":info", (":start", ":stop")[int(rng.integers(0, 2))], ":nemesis", t))
            continue
        p = int(rng.integers(0, n_procs))
        if p in open_ and u < 0.9:
            out.append(op((":ok", ":ok", ":fail", ":info")[int(rng.integers(0, 4))], open_.pop(p), p, t))
        elif u < 0.95:
            open_[p] = f":f{int(rng.integers(0, n_f))}"
            out.append(op(":invoke", open_[p], p, t))
        else:
            out.append(op(":ok", f":f{int(rng.integers(0, n_f))}", p, t))  # a lone completion
    return out


@pytest.mark.parametrize("seed", range(6))
def test_perf_report_over_the_model_equals_the_graphs(seed):
    h = random_history(seed, nemesis=seed % 2 == 0, n_procs=1 + 3 * seed)
    ops, cols = columns(h)
    res = PM.perf(*cols, arrays=True)
    assert res["unpaired"] + res["paired"] == res["invokes"]
    rep = J.perf_report(ops, {k: (np.array(v) if isinstance(v, list) else v) for k, v in res.items()})
    same_graphs(rep, PM.graphs(h))
    assert "latency_raw" in rep
    # other windows and quantiles
    res = PM.perf(*cols, qs=(0, 0.25, 0.999), q_dt=7, r_dt=3)
    rep = J.perf_report(ops, {k: (np.array(v) if isinstance(v, list) else v) for k, v in res.items()})
    same_graphs(rep, PM.graphs(h, qs=(0, 0.25, 0.999), q_dt=7, r_dt=3))


def test_with_times():
    text, _ = J.set_history_edn(3, n_adds=200, n_procs=4)
    n = len(text.strip().split("\n"))
    stamped = J.with_times(text, 5, mean_latency_ns=2_000_000, nemesis=((10, "start"), (50, "stop")))
    assert stamped == J.with_times(text, 5, mean_latency_ns=2_000_000, nemesis=((10, "start"), (50, "stop")))
    ops = J.perf_ops_from_edn(stamped)
    assert len(ops.time) == n + 4 and (np.diff(ops.time) > 0).all()
    assert [f for f, _ in ops.nemesis] == [":start", ":start", ":stop", ":stop"]
    # the ops themselves are unchanged: the set checker reads the same values
    a, b = J.set_ops_from_edn(text), J.set_ops_from_edn(stamped)
    assert np.array_equal(a.attempt, b.attempt) and np.array_equal(a.seen, b.seen)
    res = PM.perf(ops.type, ops.f, ops.process, ops.client, ops.time, len(ops.fs))
    assert res["unpaired"] == 0 and res["orphans"] == 4  # every client op pairs; the nemesis ops never do
    lat = [x for x in PM.perf(ops.type, ops.f, ops.process, ops.client, ops.time, len(ops.fs), arrays=True)["latency"] if x]
    assert 0.3 * 2_000_000 < sum(lat) / len(lat) < 3 * 2_000_000
    with pytest.raises(ValueError):
        J.with_times("[{:type :ok}\n {:type :ok}]", 1)


def test_merge_valid():
    assert J.merge_valid([True]) is True and J.merge_valid([True, True]) is True
    assert J.merge_valid([True, "unknown", True]) == "unknown"
    assert J.merge_valid(["unknown", False, True]) is False and J.merge_valid([False, "unknown"]) is False
    for bad in ([], [None], [True, "maybe"]):
        with pytest.raises(ValueError):
            J.merge_valid(bad)


def test_compose_edn_with_stub_checkers():
    seen = []

    def ok(v, text):
        seen.append((v, text))
        return {"valid": True, "x": 1}

    def boom(v, text):
        raise RuntimeError("no cluster")

    r = J.compose_edn("V", "T", {"a": ok, "b": lambda v, t: {"valid": "unknown"}})
    assert r == {"a": {"valid": True, "x": 1}, "b": {"valid": "unknown"}, "valid": "unknown"} and seen == [("V", "T")]
    r = J.compose_edn("V", "T", {"a": ok, "b": boom})
    assert r["valid"] == "unknown" and r["b"]["valid"] == "unknown" and "no cluster" in r["b"]["error"]
    assert J.compose_edn("V", "T", {"a": ok, "b": boom, "c": lambda v, t: {"valid": False}})["valid"] is False
    assert J.compose_edn("V", "T", {"a": ok})["valid"] is True
    assert set(J.COMPOSE_SETS) == {"perf", "set"} and set(J.COMPOSE_REGISTER) == {"perf", "linearizable"}
    assert set(J.compose_bank(5, 50)) == {"perf", "bank"}


# ---- the window arithmetic ------------------------------------------------------
def window_np(t, dt):
    return ((t.astype(np.float64) / 1e9) / dt).astype(np.int64)


@pytest.mark.parametrize("dt", [10, 30])
def test_windows_at_the_boundaries(dt):
    """Every time below 2^53 ns is a double, and there the two double divisions
    agree with the integer division t // (dt 10^9) at k dt 10^9 - 1, at it and
    1 ns past it, for every k (checked for all of them, about 9 10^5 / 3 10^5).
    Past 2^53 ns (104 days) a time is rounded before it is divided, and k dt
    10^9 - 1 may land in window k: the entry does the same two divisions on the
    device, so it follows the reference there too -- it accepts every window
    index below 2^32 -- and the model is the double expression throughout."""
    w = dt * S
    k = np.arange(1, ((1 << 53) - 2) // w + 1, dtype=np.int64)
    assert len(k) > 300_000
    for d in (-1, 0, 1):
        t = k * w + d
        assert t.max() < 1 << 53
        assert np.array_equal(window_np(t, dt), t // w), d
    # the model is the same expression, op by op (sampled, and the largest windows an int64 time reaches)
    top = (PM.INT64_MAX - 1) // w
    for kk in [1, 2, 1000, int(k[-1]), int(k[-1]) + 1, 1 << 22, top - 1, top]:
        for d in (-1, 0, 1):
            t = kk * w + d
            assert PM.bucket_index(dt, t) == J.bucket_of(t, dt) == int(window_np(np.array([t]), dt)[0])
            assert PM.bucket_index(dt, t) < 1 << 32
            assert PM.bucket_time(dt, PM.nanos_to_secs(t)) == J.bucket_mid(J.bucket_of(t, dt), dt)
    # where they part: 1 ns before a boundary past 2^53 ns
    t = (int(k[-1]) + 2) * w - 1
    assert t > 1 << 53 and PM.bucket_index(dt, t) == t // w + 1
