"""hsc_perf_check on the GPU (include/hip_serial.h): every field
of the report must equal the CPU model of perf_model.py -- the scalars, the
listed latency and rate cells, the counts matrix, and with the arrays every
op's completion_of / invoke_of / latency and the raw partition -- exactly, on
the shapes where a pass can go wrong: empty and tiny histories, every pairing
shape, the workgroup and scan-tile boundaries, one process or thousands, the
window boundaries up to the largest int64 time, every quantile index of cells
of 1 .. 256, the int64 extremes of a latency, the cell cap, shuffled times,
both sort paths, buffer reuse and other entries' state on the same context."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import linear_model as LM
import perf_model as PM
import resolve_model as RM
import tally_model as TM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J
from test_perf_model import random_history, same_graphs

pytestmark = pytest.mark.gpu

INV, OK, FAIL, INFO = hsc.OP_INVOKE, hsc.OP_OK, hsc.OP_FAIL, hsc.OP_INFO
SCAN_TILE = 2048  # kScanTile of scan_exclusive_u32
S = 10 ** 9
I64MAX = PM.INT64_MAX


def cols(rows, nf=None):
    """rows: (type, f, process, client, time) per op."""
    a = np.array(rows, dtype=object).reshape(-1, 5)
    c = (a[:, 0].astype(np.uint8), a[:, 1].astype(np.uint32), a[:, 2].astype(np.uint32), a[:, 3].astype(np.uint8),
         a[:, 4].astype(np.int64))
    return c + (int(c[1].max()) + 1 if nf is None and len(rows) else (nf or 1),)


def run(v, c, arrays=True, **kw):
    res = v.perf_check(*c, arrays=arrays, **kw)
    PM.assert_same_perf(res, PM.perf(*c, arrays=arrays, **kw))
    assert res["ms"] >= 0 and 0 <= res["sort_packed"] < 16 and set(res["phase_ms"]) == set(hsc.PERF_PHASES)
    return res


def pairs(n, proc=lambda i: i, f=lambda i: 0, t0=lambda i: 10 * i, lat=lambda i: 5, typ=lambda i: OK):
    """n invoke / completion pairs, the invokes first and the completions after them."""
    return [(INV, f(i), proc(i), 1, t0(i)) for i in range(n)] + \
           [(typ(i), f(i), proc(i), 1, t0(i) + lat(i)) for i in range(n)]


# ---- empty, tiny, pairing -------------------------------------------------------
def test_empty_and_tiny(validator):
    for arrays in (False, True):
        res = run(validator, cols([]), arrays)
        assert res["n"] == res["cells"] == res["rate_cells"] == res["t_max"] == 0 and res["counts"].sum() == 0
    assert run(validator, cols([(INV, 0, 0, 1, 7)]))["unpaired"] == 1
    res = run(validator, cols([(OK, 0, 0, 1, 7)]))
    assert res["orphans"] == 1 and res["rate_cells"] == 1 and res["cells"] == 0 and res["t_max"] == 7
    res = run(validator, cols([(INV, 0, 3, 1, 7), (OK, 0, 3, 1, 12)]))
    assert res["paired"] == 1 and res["latency"].tolist() == [5, 0] and res["cell_lat"].tolist() == [[5] * 4]


def test_pairing_shapes(validator):
    # inv inv ok on one process: the older invoke is unpaired
    res = run(validator, cols([(INV, 0, 0, 1, 1), (INV, 0, 0, 1, 2), (OK, 0, 0, 1, 5)]))
    assert res["completion_of"].tolist() == [-1, 2, -1] and res["unpaired"] == 1
    # inv ok ok: the second completion is an orphan
    res = run(validator, cols([(INV, 0, 0, 1, 1), (OK, 0, 0, 1, 2), (OK, 0, 0, 1, 5)]))
    assert res["invoke_of"].tolist() == [-1, 0, -1] and res["orphans"] == 1
    # two processes interleaved, one completing :info, one :fail
    res = run(validator, cols([(INV, 0, 0, 1, 1), (INV, 1, 1, 1, 2), (INFO, 0, 0, 1, 9), (FAIL, 1, 1, 1, 4)]))
    assert res["completion_of"].tolist() == [2, 3, -1, -1] and res["latency"].tolist() == [8, 2, 0, 0]
    # nemesis ops are :info on both sides and never pair; an interned non-integer process pairs like any other
    res = run(validator, cols([(INFO, 2, 9, 0, 1), (INV, 0, 4, 0, 2), (INFO, 2, 9, 0, 3), (OK, 0, 4, 0, 6)]))
    assert res["paired"] == 1 and res["orphans"] == 2 and res["rate_cells"] == 0 and res["counts"][2][INFO] == 2
    # an invoke after a completion of another process with the same times
    run(validator, cols([(OK, 0, 1, 1, 5), (INV, 0, 1, 1, 5), (INV, 0, 2, 1, 5), (OK, 0, 2, 1, 5)]))


# ---- workgroup and scan-tile boundaries -------------------------------------------
def test_a_pair_across_a_workgroup_boundary(validator):
    # after the process sort: 255 lone completions of process 0, then process 1's invoke at 255, its completion at 256
    rows = [(OK, 0, 0, 1, 10 + i) for i in range(255)]
    rows.insert(100, (INV, 1, 1, 1, 50))
    rows.insert(200, (FAIL, 1, 1, 1, 90))
    res = run(validator, cols(rows))
    assert res["paired"] == 1 and res["completion_of"][100] == 200 and res["latency"][100] == 40
    # and the same split the other way round: the completion is a workgroup's first row
    rows = [(INV, 1, 1, 1, 50)] + [(INV, 0, 0, 1, 10 + i) for i in range(254)] + [(OK, 0, 0, 1, 999), (OK, 1, 1, 1, 60)]
    assert run(validator, cols(rows))["paired"] == 2


@pytest.mark.parametrize("total", [255, 256, 257, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_totals_at_the_block_and_scan_tile_boundaries(validator, total):
    run(validator, random_cols(total, total, n_procs=7, n_f=3))


# ---- process shapes -------------------------------------------------------------
def test_one_process_owns_every_op(validator):
    rng = np.random.default_rng(1)
    types = rng.choice([INV, INV, OK, FAIL, INFO], 3000)
    rows = [(int(t), int(rng.integers(0, 2)), 5, 1, 1000 * i) for i, t in enumerate(types)]
    res = run(validator, cols(rows))
    assert res["paired"] > 500 and res["unpaired"] > 100 and res["orphans"] > 100


def test_5000_processes_one_pair_each(validator):
    rng = np.random.default_rng(2)
    ids = rng.permutation(1 << 20)[:5000]
    order = rng.permutation(5000)
    res = run(validator, cols(pairs(5000, proc=lambda i: int(ids[order[i]]) * 4093, lat=lambda i: i)))
    assert res["paired"] == 5000 and res["orphans"] == 0


# ---- windows ----------------------------------------------------------------------
def test_window_boundaries(validator):
    rows, p = [], 0
    for dt in (30, 10):
        top = (I64MAX - 1) // (dt * S)
        for k in (1, 2, 1 << 22, top):  # (2^22 windows: past 2^53 ns, where the doubles and integer division part)
            for d in (-1, 0, 1):
                t = k * dt * S + d
                rows += [(INV, 0, p, 1, t), (OK, 0, p, 1, t)]
                p += 1
    res = run(validator, cols(rows))
    assert res["t_max"] == ((I64MAX - 1) // (10 * S)) * 10 * S + 1
    assert int(res["cell_bucket"].max()) == PM.bucket_index(30, int(res["t_max"]))
    # and under other windows, fractional ones too
    run(validator, cols(rows), q_dt=2.5, r_dt=7)
    run(validator, cols([(INV, 0, 0, 1, 1), (OK, 0, 0, 1, I64MAX)]), q_dt=2.15, r_dt=2.15)


# ---- quantiles, latencies, cells ----------------------------------------------------
def test_quantile_index_of_every_cell_size(validator):
    rng = np.random.default_rng(3)
    rows, p = [], 0
    for size in range(1, 257):  # a cell of every size, each in a window of its own
        for lat in rng.integers(0, 10 ** 7, size).tolist():
            rows += [(INV, size % 3, p, 1, size * 30 * S + p), (OK, size % 3, p, 1, size * 30 * S + p + lat)]
            p += 1
    qs = (0.5, 0.95, 0.99, 1, 0, 0.999)
    res = run(validator, cols(rows), arrays=False, qs=qs)
    assert res["cells"] == 256 and sorted(res["cell_count"].tolist()) == list(range(1, 257))
    assert (res["cell_lat"][:, 4] <= res["cell_lat"][:, 0]).all() and (res["cell_lat"][:, 5] <= res["cell_lat"][:, 3]).all()


def test_latencies_equal_negative_and_extreme(validator):
    res = run(validator, cols(pairs(700, lat=lambda i: 12345, t0=lambda i: i)))
    assert (res["cell_lat"] == 12345).all()
    # a hand-made history with completions before their invokes: negative latencies, kept
    res = run(validator, cols(pairs(300, lat=lambda i: -1000 * i, t0=lambda i: S + i)))
    assert res["cell_lat"][0].tolist() == [-149000, -14000, -2000, 0]
    rows = [(INV, 0, 0, 1, 0), (OK, 0, 0, 1, I64MAX), (INV, 0, 1, 1, I64MAX), (OK, 0, 1, 1, 0),
            (INV, 0, 2, 1, 5), (OK, 0, 2, 1, 6), (INV, 0, 3, 1, I64MAX), (OK, 0, 3, 1, I64MAX)]
    res = run(validator, cols(rows), qs=(0, 1))
    assert res["latency"].tolist() == [I64MAX, 0, -I64MAX, 0, 1, 0, 0, 0]
    assert res["cell_lat"].tolist() == [[1, I64MAX], [-I64MAX, 0]]


def test_one_cell_across_workgroups_and_many_cells_of_one(validator):
    rng = np.random.default_rng(4)
    lat = rng.integers(0, 10 ** 6, 5000)
    res = run(validator, cols(pairs(5000, lat=lambda i: int(lat[i]), t0=lambda i: i)))
    assert res["cells"] == 1 and res["cell_count"].tolist() == [5000]
    assert res["cell_lat"][0].tolist() == [int(np.sort(lat)[i]) for i in (2500, 4750, 4950, 4999)]
    res = run(validator, cols(pairs(5000, t0=lambda i: int(rng.integers(0, 2)) + 30 * S * i, f=lambda i: i % 2)))
    assert res["cells"] == 5000 and (res["cell_count"] == 1).all()


def test_more_cells_than_the_cap(validator):
    n = hsc.PERF_CELL_CAP + 500
    c = cols(pairs(n, t0=lambda i: i * S, lat=lambda i: 1000))
    res = run(validator, c, arrays=False, q_dt=1, r_dt=1)
    assert res["cells"] == res["rate_cells"] == n and res["cells_listed"] == res["rate_listed"] == hsc.PERF_CELL_CAP
    assert res["cell_bucket"].tolist() == list(range(hsc.PERF_CELL_CAP))
    ops = J.PerfOps(*c[:5], fs=[":add"], processes=list(range(n)), nemesis=[])
    assert J.perf_report(ops, res)["truncated"] == ["latency_quantiles", "rate"]


# ---- rate -------------------------------------------------------------------------
def test_rate_cells(validator):
    # every (f, type) pair occupied, a few windows each
    rows = [(t, f, 10 * f + t, 1, (f + 3 * t + 7 * k) * S) for f in range(4) for t in (OK, FAIL, INFO) for k in range(5)]
    res = run(validator, cols(rows))
    assert (res["counts"][:, 1:] == 5).all() and (res["counts"][:, 0] == 0).all() and res["rate_cells"] > 12
    # a client = 0 completion is counted in counts and absent from rate, even in a window clients share
    rows = [(OK, 0, 1, 1, 3 * S), (INFO, 0, 9, 0, 4 * S), (OK, 0, 9, 0, 5 * S), (INFO, 1, 9, 0, 25 * S)]
    res = run(validator, cols(rows))
    assert res["rate_count"].tolist() == [1] and res["counts"].tolist() == [[0, 2, 0, 1], [0, 0, 0, 1]]
    # the t-max rule: the completion at 12 s lies past the last listed midpoint (5 s)
    rows = [(INV, 0, 1, 1, 1 * S), (OK, 0, 1, 1, 2 * S), (INV, 0, 1, 1, 3 * S), (OK, 0, 1, 1, 12 * S)]
    c = cols(rows)
    res = run(validator, c)
    assert res["rate_bucket"].tolist() == [0, 1]
    ops = J.PerfOps(*c[:5], fs=[":r"], processes=[0, 1], nemesis=[])
    rep = J.perf_report(ops, res)
    assert rep["rate"] == {":r": {":ok": [(5, 0.1)], ":info": [(5, 0)], ":fail": [(5, 0)]}}
    same_graphs(rep, PM.graphs(PM.history_of(*c[:5], fs=[":r"])))


def test_shuffled_times(validator):
    c = random_cols(6, 6000, n_procs=16, n_f=4, span=3600 * S)
    rng = np.random.default_rng(6)
    shuffled = c[:4] + (rng.permutation(c[4]),) + c[5:]
    res = run(validator, shuffled)
    assert (res["latency"] < 0).any() and res["rate_cells"] > 1000


def test_both_sort_paths(validator):
    rng = np.random.default_rng(9)
    small = rng.integers(0, 500, 1500)
    wide = rng.integers(0, I64MAX, 1500, dtype=np.int64)
    took = set()
    for lat in (small, wide):
        # (the invokes at 0 and the completions at the latency itself: latencies over 63 bits leave the row index no room)
        rows = [(INV, 0, i, 1, 0) for i in range(1500)] + [(OK, 0, i, 1, int(lat[i])) for i in range(1500)]
        took.add(run(validator, cols(rows), q_dt=2.15, r_dt=2.15)["sort_packed"] & 2)
    assert took == {0, 2}


# ---- context hygiene -------------------------------------------------------------------
def test_buffer_reuse_large_small_large(validator):
    for seed, n in ((21, 120_000), (22, 10), (23, 150_000), (24, 7)):
        c = random_cols(seed, n, n_procs=32, n_f=5)
        res = validator.perf_check(*c, arrays=True)
        if n < 1000:
            PM.assert_same_perf(res, PM.perf(*c, arrays=True))
        else:  # (the model in plain Python on 10^5 ops: the scalars and the pairing through numpy instead)
            inv = np.flatnonzero(res["completion_of"] >= 0)
            assert res["paired"] == len(inv) and (res["invoke_of"][res["completion_of"][inv]] == inv).all()
            assert np.array_equal(res["latency"][inv], c[4][res["completion_of"][inv]] - c[4][inv])
            assert res["counts"].sum() == (c[0] != INV).sum() and res["cell_count"].sum() == res["paired"]


def test_perf_between_a_resolve_and_its_build(validator):
    v = validator
    h = RM.generated(11, n_txn=800, n_keys=80)
    edges = lambda: [a.copy() for a in v.dep_graph_edges()]  # noqa: E731
    v.dep_graph_resolve(h, arrays=False)
    v.dep_graph_build_resolved(full=True)
    want = edges()
    assert len(want[0]) > 0
    v.dep_graph_resolve(h, arrays=False)
    run(v, random_cols(12, 20_000, n_procs=9, n_f=3))  # more rows than the history has ops
    v.dep_graph_build_resolved(full=True)
    for x, y in zip(edges(), want):
        np.testing.assert_array_equal(x, y)


def test_interleaved_with_linear_and_tally_checks(validator):
    ops = LM.columns([LM.concurrent_writes(3), LM.concurrent_writes(2, read=9)])
    want = LM.check(ops, None)
    rng = np.random.default_rng(4)
    vals = rng.integers(0, 50, 700)
    tally = TM.tally(vals[:300], vals[200:500], vals[400:], True)
    for i in range(3):
        LM.assert_same(validator.linear_check(ops, None), want)
        run(validator, random_cols(40 + i, 900, n_procs=4, n_f=2))
        TM.assert_same_tally(validator.tally_check(vals[:300], vals[200:500], vals[400:], multiset=True), tally)
    LM.assert_same(validator.linear_check(ops, None), want)


# ---- random histories ---------------------------------------------------------------
def random_cols(seed, n_ops, n_procs, n_f, nemesis=True, span=600 * S):
    """Columns of a history with every pairing shape at sorted random times;
    the nemesis is process id n_procs, client 0."""
    rng = np.random.default_rng(1000 + seed)
    time = np.sort(rng.integers(0, span, n_ops)).astype(np.int64)
    proc = rng.integers(0, n_procs, n_ops).astype(np.uint32)
    typ = np.zeros(n_ops, np.uint8)
    f = np.zeros(n_ops, np.uint32)
    client = np.ones(n_ops, np.uint8)
    u = rng.random(n_ops)
    pick = rng.integers(0, n_f, n_ops)
    ctype = rng.choice([OK, OK, OK, FAIL, INFO], n_ops)
    open_ = {}
    for i in range(n_ops):
        p = int(proc[i])
        if nemesis and u[i] < 0.01:
            proc[i], client[i], typ[i], f[i] = n_procs, 0, INFO, n_f - 1
        elif p in open_ and u[i] < 0.93:
            typ[i], f[i] = ctype[i], open_.pop(p)
        elif u[i] < 0.97:
            typ[i], f[i] = INV, pick[i]
            open_[p] = int(pick[i])
        else:
            typ[i], f[i] = ctype[i], pick[i]  # a lone completion
    return typ, f, proc, client, time, n_f


@pytest.mark.parametrize("seed,n_ops,n_procs,n_f,nemesis", [(0, 20_000, 64, 6, True), (1, 20_000, 1, 1, False),
                                                             (2, 5000, 5, 3, True), (3, 9000, 17, 2, False),
                                                             (4, 3000, 64, 6, True), (5, 1500, 2, 4, True)])
def test_random(validator, seed, n_ops, n_procs, n_f, nemesis):
    res = run(validator, random_cols(seed, n_ops, n_procs, n_f, nemesis), arrays=seed % 2 == 0)
    assert res["paired"] > n_ops // 4 and (n_procs == 1 or res["unpaired"] > 0) and res["orphans"] > 0


# ---- EDN level -------------------------------------------------------------------------
def model_report(text, **kw):
    ops = J.perf_ops_from_edn(text)
    res = PM.perf(ops.type, ops.f, ops.process, ops.client, ops.time, max(len(ops.fs), 1), **kw)
    return J.perf_report(ops, {k: (np.array(v) if isinstance(v, list) else v) for k, v in res.items()})


def same_perf_report(got, want):
    assert got.keys() == want.keys()
    for k in want:
        if k == "perf":
            PM.assert_same_perf(got[k], want[k])
        else:
            assert got[k] == want[k], k


def stamped(kind):
    if kind == "set":
        text = J.set_history_edn(7, n_adds=400, n_procs=5, info_frac=0.05)[0]
    elif kind == "bank":
        text = J.bank_history_edn(13, n=5, start=10, n_ops=300, n_procs=4)[0]
    else:
        text = J.cas_register_history_edn(5, n_ops=300, n_procs=5)[0]
    return J.with_times(text, 3, mean_latency_ns=400_000_000, nemesis=((50, "start"), (200, "stop"), (400, "start")))


@pytest.mark.parametrize("kind", ["set", "bank", "register"])
@pytest.mark.parametrize("arrays", [False, True])
def test_check_perf_edn(validator, kind, arrays):
    text = stamped(kind)
    rep = J.check_perf_edn(validator, text, arrays=arrays)
    same_perf_report(rep, model_report(text, arrays=arrays))
    assert rep["valid"] is True and rep["paired"] > 100 and len(rep["nemesis_intervals"]) == 4
    assert ("latency_raw" in rep) == arrays
    same_graphs(rep, PM.graphs([{"type": o[":type"], "f": o[":f"], "process": o[":process"], "time": o[":time"]}
                                for o in J.parse_edn(text)]))
    rep = J.check_perf_edn(validator, text, qs=(0.5,), q_dt=5, r_dt=2)
    same_perf_report(rep, model_report(text, qs=(0.5,), q_dt=5, r_dt=2))


def test_compose_presets(validator):
    r = J.compose_edn(validator, stamped("set"), J.COMPOSE_SETS)
    assert set(r) == {"perf", "set", "valid"} and r["valid"] is True and r["perf"]["valid"] is True
    lossy = J.with_times(J.set_history_edn(7, n_adds=400, n_procs=5, lose=3)[0], 3)
    r = J.compose_edn(validator, lossy, J.COMPOSE_SETS)
    assert r["valid"] is False and r["set"]["valid"] is False and r["perf"]["valid"] is True
    assert r["set"]["lost_count"] == 3 and r["perf"]["unpaired"] == 0
    r = J.compose_edn(validator, stamped("register"), J.COMPOSE_REGISTER)
    assert set(r) == {"perf", "linearizable", "valid"} and r["valid"] == r["linearizable"]["valid"]
    r = J.compose_edn(validator, stamped("bank"), J.compose_bank(5, 50))
    assert set(r) == {"perf", "bank", "valid"} and r["valid"] is True and r["bank"]["valid"] is True
    skewed = J.with_times(J.bank_history_edn(13, n=5, start=10, n_ops=300, n_procs=4, skew_reads=2)[0], 3)
    assert J.compose_edn(validator, skewed, J.compose_bank(5, 50))["valid"] is False
    # a member that raises (a history without :time) is "unknown", the others still run
    r = J.compose_edn(validator, J.set_history_edn(7, n_adds=50)[0], J.COMPOSE_SETS)
    assert r["perf"]["valid"] == "unknown" and "time" in r["perf"]["error"] and r["set"]["valid"] is True
    assert r["valid"] == "unknown"


# ---- invalid input -----------------------------------------------------------------------
def test_invalid_input(validator):
    v = validator
    good = cols([(INV, 0, 0, 1, 1), (OK, 1, 0, 1, 2)])
    run(v, good)

    def bad(c=good, **kw):
        with pytest.raises(hsc.HscError):
            v.perf_check(*c, **kw)

    bad(good[:5] + (1,))                                           # an f >= nf
    bad(good[:5] + (0,))                                           # nf of 0
    bad(good[:5] + (hsc.PERF_MAX_F + 1,))
    bad((np.array([0, 4], np.uint8),) + good[1:])                  # a type above info
    bad(good[:4] + (np.array([1, -1], np.int64),) + good[5:])      # a negative time
    bad(good[:4] + (np.array([1, 1 << 62], np.int64),) + good[5:], r_dt=1)   # past the accepted windows
    bad(good[:4] + (np.array([1, 1 << 62], np.int64),) + good[5:], q_dt=0.5)
    for q in (-0.1, 1.5, float("nan")):
        bad(qs=(0.5, q))
    bad(qs=[0.5] * (hsc.PERF_MAX_Q + 1))
    for dt in (0, -1, float("inf"), float("nan")):
        bad(q_dt=dt)
        bad(r_dt=dt)
    lib, ctx = v.lib, v.ctx
    import ctypes as C
    s = hsc._PerfIn(0, None, None, None, None, None, 1, 0, None, 30.0, 10.0)
    rep = hsc.PerfReport()
    assert lib.hsc_perf_check(ctx, C.byref(s), 0, C.byref(rep)) == hsc.HSC_OK and rep.counts
    assert lib.hsc_perf_check(ctx, C.byref(s), 2, C.byref(rep)) != hsc.HSC_OK       # an unknown flag
    assert lib.hsc_perf_check(ctx, None, 0, C.byref(rep)) != hsc.HSC_OK             # NULL arguments
    assert lib.hsc_perf_check(ctx, C.byref(s), 0, None) != hsc.HSC_OK
    assert lib.hsc_perf_check(None, C.byref(s), 0, C.byref(rep)) != hsc.HSC_OK
    s.n = 2
    assert lib.hsc_perf_check(ctx, C.byref(s), 0, C.byref(rep)) != hsc.HSC_OK       # NULL arrays with n > 0
    s.n = 0x80000000  # past what the u32 scans carry (refused before any array is read)
    for name, a in zip(("type", "f", "process", "client", "time"), good[:5]):
        setattr(s, name, a.ctypes.data)
    assert lib.hsc_perf_check(ctx, C.byref(s), 0, C.byref(rep)) != hsc.HSC_OK
    s.n, s.nq = 2, 1
    assert lib.hsc_perf_check(ctx, C.byref(s), 0, C.byref(rep)) != hsc.HSC_OK       # nq without q
    run(v, good)  # the context still works
