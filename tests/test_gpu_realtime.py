"""GPU: the real-time order as dependency edges (hsc_dep_graph_stage_realtime,
comdb2_amd/csrc/hsc_realtime.hip) -- the staged edges against
the CPU model of the transitive reduction (realtime_model.py), the staging
rules, the components against Tarjan over the FULL relation, the anomaly
classes over the widened E1 against test_anomaly's reference, and the Jepsen
report's strict-serializability verdict."""
import functools
import os

import numpy as np
import pytest
import torch  # imported before any test initialises HIP

import realtime_model as M
from comdb2_amd import hsc
from comdb2_amd import jepsen as J
from comdb2_amd.workloads import History, config4_history
from test_anomaly import (G2, GSINGLE, SERIAL, WRITE_SKEW, assert_matches, check_witnesses, hist,
                          ref_anomalies, with_future_reads)

pytestmark = pytest.mark.gpu

EINVAL = r"-> %d:" % hsc.HSC_EINVAL
# the kernels' constants (hsc_realtime.hip, hsc_kernels.hip)
RT_TILE = 256            # kRtTile = kRtThreads: a suffix tile, a count / emit workgroup
RT_TOP = 256 * RT_TILE   # kRtTop tiles: one step of the second suffix level
SCAN_TILE = 2048         # kScanTile: the count scan runs over ntxn + 1 words
SORT_TILE = 4096         # kSortTile: a workgroup of the radix passes
SORT_SCAN = 8 * SORT_TILE  # 256 digit counters x 8 workgroups = one scan tile of the sort's counts


def no_ops(n):
    return History(np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint8),
                   np.zeros(0, np.int64), n)


def staged(v, inv, cpl):
    """Stage, build a history of no ops, return (stage dict, src, dst, type)."""
    st = v.dep_graph_stage_realtime(inv, cpl)
    v.dep_graph_build(no_ops(len(inv)), full=True)
    return (st,) + v.dep_graph_edges()


def assert_edges(got, want_s, want_d):
    st, s, d, t = got
    assert st["edges"] == len(want_s) and st["ms"] > 0
    np.testing.assert_array_equal(s, want_s)
    np.testing.assert_array_equal(d, want_d)
    assert (t == 8).all()


# ---------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------
def test_every_small_size_matches_the_literal_model(validator):
    for n in range(1, 71):
        inv, cpl = M.random_intervals(n, n, procs=4, open_frac=0.15 if n % 3 == 0 else 0.0)
        assert_edges(staged(validator, inv, cpl), *M.pairs(M.reduced(inv, cpl)))


def test_sequential_history_is_a_chain(validator):
    n = 700
    inv = 2 * np.arange(n, dtype=np.uint64)
    st, s, d, t = got = staged(validator, inv, inv + np.uint64(1))
    assert_edges(got, *M.pairs(M.reduced(inv, inv + np.uint64(1))))
    assert st["edges"] == n - 1
    np.testing.assert_array_equal(d, s + 1)


def test_overlapping_intervals_have_no_order(validator):
    n = 700
    inv = np.arange(n, dtype=np.uint64)
    st, s, d, t = staged(validator, inv, inv + np.uint64(1000))
    assert st["edges"] == 0 and len(s) == 0


def test_times_tied_in_pairs(validator):
    n = 600
    rng = np.random.default_rng(5)
    inv = (10 * (np.arange(n) // 2)).astype(np.uint64)
    cpl = inv + np.uint64(5)
    perm = rng.permutation(n)
    inv, cpl = inv[perm], cpl[perm]
    got = staged(validator, inv, cpl)
    assert_edges(got, *M.pairs(M.reduced(inv, cpl)))
    assert got[0]["edges"] == 4 * (n // 2 - 1)  # each pair precedes the next pair, both ways
    # and every time tied: nothing precedes anything
    st, s, d, t = staged(validator, np.full(n, 7, np.uint64), np.full(n, 7, np.uint64))
    assert st["edges"] == 0


def test_a_third_of_the_completions_open(validator):
    inv, cpl = M.random_intervals(11, 1500, procs=6, open_frac=1 / 3)
    assert 400 < int((cpl == M.OPEN).sum()) < 600
    got = staged(validator, inv, cpl)
    assert_edges(got, *M.pairs(M.reduced(inv, cpl)))
    assert not np.isin(got[1], np.nonzero(cpl == M.OPEN)[0]).any()  # an open txn precedes nothing


BOUNDARIES = sorted({b + k for b in (RT_TILE, SCAN_TILE - 1, SORT_TILE, SORT_SCAN, RT_TOP) for k in (-1, 0, 1)}
                    | {2 * RT_TILE + 1, 70001})


@pytest.mark.parametrize("n", BOUNDARIES)
def test_block_and_grid_boundaries(validator, n):
    inv, cpl = M.random_intervals(n, n, procs=8, open_frac=0.1, step=5)
    ws, wd = M.reduced_sorted(inv, cpl)
    if n <= SCAN_TILE + 1:  # the literal model while its matrix is small
        ls, ld = M.pairs(M.reduced(inv, cpl))
        np.testing.assert_array_equal(ws, ls)
        np.testing.assert_array_equal(wd, ld)
    assert_edges(staged(validator, inv, cpl), ws, wd)


@pytest.mark.parametrize("n", [RT_TILE + 3, RT_TOP + 300])
def test_minimum_carried_across_every_tile(validator, n):
    """Txn 0 completes first; every other txn but the last is open; the last
    completes after all were invoked.  Txn 0's first-completion search finds
    its minimum in the last tile, through the second suffix level (and, at the
    larger size, its carry from one step to the next); it precedes them all."""
    inv = np.arange(n, dtype=np.uint64) + np.uint64(10)
    cpl = np.full(n, M.OPEN, np.uint64)
    inv[0], cpl[0] = 0, 1
    cpl[n - 1] = 10 + 2 * n
    st, s, d, t = got = staged(validator, inv, cpl)
    assert_edges(got, *M.reduced_sorted(inv, cpl))
    assert st["edges"] == n - 1 and (s == 0).all()


# ---------------------------------------------------------------------------
# errors and staging
# ---------------------------------------------------------------------------
def plain_edges(v, oracle_mod, h):
    v.dep_graph_build(h, full=True)
    s, d, t = v.dep_graph_edges()
    ws, wd, wt = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
    np.testing.assert_array_equal(s, ws)
    np.testing.assert_array_equal(d, wd)
    np.testing.assert_array_equal(t, wt)


def test_errors_and_staging_rules(validator, oracle_mod):
    v = validator
    h = config4_history(seed=2, n_txn=300, n_keys=40, concurrent_frac=0.2, max_lag=6)
    inv, cpl = M.random_intervals(3, 300, procs=4)
    # a txn completing before its invoke
    bad = inv.copy()
    bad[17] = cpl[17] + np.uint64(1)
    with pytest.raises(hsc.HscError, match=EINVAL):
        v.dep_graph_stage_realtime(bad, cpl)
    plain_edges(v, oracle_mod, h)  # nothing was staged
    # a build of another ntxn: fails, drops the staged edges
    assert v.dep_graph_stage_realtime(inv[:299], cpl[:299])["edges"] > 0
    with pytest.raises(hsc.HscError, match=EINVAL):
        v.dep_graph_build(h, full=True)
    plain_edges(v, oracle_mod, h)
    # no txns
    assert v.dep_graph_stage_realtime(np.zeros(0, np.uint64), np.zeros(0, np.uint64))["edges"] == 0
    v.dep_graph_build(no_ops(0), full=True)
    assert len(v.dep_graph_edges()[0]) == 0
    # staging twice replaces
    other = M.random_intervals(4, 300, procs=2)
    v.dep_graph_stage_realtime(*other)
    assert_edges(staged(v, inv, cpl), *M.pairs(M.reduced(inv, cpl)))
    # consumed by one build
    v.dep_graph_build(no_ops(300), full=True)
    assert len(v.dep_graph_edges()[0]) == 0
    plain_edges(v, oracle_mod, h)
    # merged with the history's own edges: types OR-ed
    v.dep_graph_stage_realtime(inv, cpl)
    v.dep_graph_build(h, full=True)
    rs, rd = M.pairs(M.reduced(inv, cpl))
    want = M.merged_edges(300, oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed), (rs, rd, 8))
    for g, w in zip(v.dep_graph_edges(), want):
        np.testing.assert_array_equal(g, w)
    assert ((want[2] & 8) != 0).any() and ((want[2] & 8 != 0) & (want[2] & 7 != 0)).any()


@pytest.mark.parametrize("first", ["rw", "rt"])
def test_rw_pairs_and_the_order_staged_together(oracle_mod, first):
    """tests/test_graph.py's staged-pairs case with the real-time order beside
    it: either staging order, a second staging of one kind replacing that kind
    only; the merged edge list is the union computed on the CPU."""
    from comdb2_amd.workloads import history_window, int64_words
    h = config4_history(n_txn=3000, n_keys=200, concurrent_frac=0.3, max_lag=16)
    hw = history_window(h)
    inv, cpl = commit_order_intervals(h.ntxn, 0)
    ids = np.arange(h.ntxn)
    v = hsc.Validator(0)
    try:
        v.register_group("t1", 0, 9)
        dev = torch.device("cuda", 0)
        gid = torch.zeros(len(hw.keys), dtype=torch.int32, device=dev)
        words = torch.from_numpy(int64_words(hw.keys).reshape(-1).view(np.int64)).to(dev)
        lsn = torch.from_numpy(hw.lsn.view(np.int64)).to(dev)
        v.ingest_device(len(hw.keys), 2, gid.data_ptr(), words.data_ptr(), lsn.data_ptr(), hw.end_lsn)
        torch.cuda.synchronize()
        txn, wl = v.rw_edges(hw.readsets)
        assert len(txn) > 0
        if first == "rw":
            v.dep_graph_stage_rw_pairs(ids, hw.commit_lsn, ids)
            v.dep_graph_stage_realtime(*M.random_intervals(1, h.ntxn))  # replaced below
            v.dep_graph_stage_realtime(inv, cpl)
        else:
            v.dep_graph_stage_realtime(inv, cpl)
            v.dep_graph_stage_rw_pairs(ids[::-1], hw.commit_lsn, ids)  # replaced below
            v.dep_graph_stage_rw_pairs(ids, hw.commit_lsn, ids)
        v.dep_graph_build(h, full=True, no_rw=True)
        got = v.dep_graph_edges()
        s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
        own = (t & 3) != 0  # a no_rw build's own edges: ww and wr
        writer = np.searchsorted(hw.commit_lsn, wl)
        np.testing.assert_array_equal(hw.commit_lsn[writer], wl)
        want = M.merged_edges(h.ntxn, (s[own], d[own], t[own] & 3), (txn, writer, 4),
                              M.reduced_sorted(inv, cpl) + (8,))
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
        assert all(((want[2] & b) != 0).any() for b in (1, 2, 4, 8))
        # both kinds were consumed
        v.dep_graph_build(no_ops(h.ntxn), full=True)
        assert len(v.dep_graph_edges()[0]) == 0
    finally:
        v.close()


# ---------------------------------------------------------------------------
# components and anomaly classes
# ---------------------------------------------------------------------------
def commit_order_intervals(n, seed, max_span=12):
    """Intervals consistent with txn id = commit order: complete = 2 id + 1,
    invoke = complete - a random span."""
    rng = np.random.default_rng(seed)
    cpl = 2 * np.arange(n, dtype=np.int64) + 1
    inv = np.maximum(cpl - rng.integers(0, max_span + 1, size=n), 0)
    return inv.astype(np.uint64), cpl.astype(np.uint64)


@functools.lru_cache(maxsize=None)
def case(n):
    h = config4_history(seed=n, n_txn=n, n_keys=n // 15, concurrent_frac=0.1, max_lag=6)
    h = with_future_reads(h, 0.01, n)
    inv, cpl = commit_order_intervals(n, n)
    return h, inv, cpl


_REF = {}


def reference(oracle_mod, n):
    """(scc over the history's edges and the FULL relation, ref_anomalies over
    the edges the build holds -- the history's and the reduction, types
    remapped --, those edges with their own types)."""
    if n not in _REF:
        h, inv, cpl = case(n)
        dep = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
        fs, fd, _ = M.merged_edges(n, dep, M.pairs(M.full(inv, cpl)) + (8,))
        edges = M.merged_edges(n, dep, M.pairs(M.reduced(inv, cpl)) + (8,))
        ref = ref_anomalies(oracle_mod, n, edges[0], edges[1], M.remap_types(edges[2]))
        _REF[n] = (oracle_mod.scc(n, fs, fd), ref, edges)
    return _REF[n]


def build_strict(v, h, inv, cpl):
    st = v.dep_graph_stage_realtime(inv, cpl)
    v.dep_graph_build(h, full=True)
    return st


@pytest.mark.parametrize("n", [1500, 3000])
def test_components_equal_tarjan_over_the_full_relation(validator, oracle_mod, n):
    h, inv, cpl = case(n)
    scc_full, ref, edges = reference(oracle_mod, n)
    build_strict(validator, h, inv, cpl)
    for g, w in zip(validator.dep_graph_edges(), edges):
        np.testing.assert_array_equal(g, w)
    scc, st = validator.dep_graph_scc_built(n)
    np.testing.assert_array_equal(scc, scc_full)
    np.testing.assert_array_equal(scc, ref.scc)
    assert st["nontrivial_sccs"] > 0
    # the order adds cycles the plain graph does not have
    plain = oracle_mod.scc(n, *oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)[:2])
    assert (scc != plain).any()


@pytest.mark.parametrize("n", [1500, 3000])
def test_anomaly_classes_over_the_widened_e1(validator, oracle_mod, n):
    h, inv, cpl = case(n)
    _, ref, edges = reference(oracle_mod, n)
    build_strict(validator, h, inv, cpl)
    res = validator.dep_graph_anomalies()
    assert_matches(res, ref, n)
    assert ref.comps[0] > 0 and ref.comps[1] > 0 and ref.anti_edges > 0  # G1c and G-single components
    check_witnesses(dict(res, wit_type=M.remap_types(res["wit_type"]).astype(np.uint8)), ref)
    # the witnesses carry the build's own type words
    edge = {(int(a), int(b)): int(t) for a, b, t in zip(*edges)}
    off, tx, ty = res["wit_off"], res["wit_txn"].tolist(), res["wit_type"].tolist()
    for c in range(len(res["comp_label"])):
        cyc = tx[off[c]:off[c + 1]]
        assert [edge[(a, b)] for a, b in zip(cyc, cyc[1:] + cyc[:1])] == ty[off[c]:off[c + 1]]
    assert any(t & 8 for t in ty)


# ---------------------------------------------------------------------------
# hand-built cases
# ---------------------------------------------------------------------------
def seq(n):
    inv = 2 * np.arange(n, dtype=np.uint64)
    return inv, inv + np.uint64(1)


def both_passes(v, h, inv, cpl):
    v.dep_graph_build(h, full=True)
    plain = v.dep_graph_anomalies()
    build_strict(v, h, inv, cpl)
    return plain, v.dep_graph_anomalies(), v.dep_graph_edges()


def test_stale_read_is_a_gsingle_only_in_real_time(validator):
    # w1 commits, w2 commits, then a read is invoked and returns w1's value
    h = hist([(0, 1, "w"), (1, 1, "w"), (2, 1, "r", 0)], 3)
    plain, strict, (s, d, t) = both_passes(validator, h, *seq(3))
    assert len(plain["comp_label"]) == 0 and not plain["cls"].any()
    assert list(zip(s.tolist(), d.tolist(), t.tolist())) == [(0, 1, 1 | 8), (0, 2, 2), (1, 2, 8), (2, 1, 4)]
    assert strict["comp_label"].tolist() == [2] and strict["comp_class"].tolist() == [GSINGLE]
    assert strict["cls"].tolist() == [0, GSINGLE | G2, GSINGLE | G2]
    # the cycle: the closing edge r -> w2 is the anti edge, w2 -> r real time
    assert strict["wit_txn"].tolist() == [1, 2] and strict["wit_type"].tolist() == [8, 4]


def test_sequential_write_skew_becomes_gsingle(validator):
    plain, strict, (s, d, t) = both_passes(validator, WRITE_SKEW, *seq(2))
    assert plain["comp_class"].tolist() == [G2] and plain["cls"].tolist() == [G2, G2]
    # T1 -> T2 is rw and real time: E1.  T2 -> T1 stays the one anti edge.
    assert list(zip(s.tolist(), d.tolist(), t.tolist())) == [(0, 1, 4 | 8), (1, 0, 4)]
    assert strict["comp_class"].tolist() == [GSINGLE] and strict["cls"].tolist() == [GSINGLE | G2] * 2
    assert strict["wit_txn"].tolist() == [0, 1] and strict["wit_type"].tolist() == [12, 4]
    # run concurrently instead, the order adds nothing: still G2
    _, conc, _ = both_passes(validator, WRITE_SKEW, np.array([0, 1], np.uint64), np.array([5, 6], np.uint64))
    assert conc["comp_class"].tolist() == [G2]


def test_strict_serializable_history_has_no_component(validator):
    plain, strict, (s, d, t) = both_passes(validator, SERIAL, *seq(3))
    assert len(plain["comp_label"]) == 0 and len(strict["comp_label"]) == 0
    assert not strict["cls"].any() and (t & 8).any()


# ---------------------------------------------------------------------------
# Jepsen report
# ---------------------------------------------------------------------------
STALE = "\n".join([
    "{:type :invoke :f :write :value 1 :process 0 :uid 1 :time 10}",
    "{:type :ok :f :write :process 0 :value 1 :uid 1 :time 20}",
    "{:type :invoke :f :write :value 2 :process 1 :uid 2 :time 30}",
    "{:type :ok :f :write :process 1 :value 2 :uid 2 :time 40}",
    "{:type :invoke :f :read :value nil :process 2 :time 50}",
    "{:type :invoke :f :read :value nil :process 3 :time 55}",
    "{:type :ok :f :read :process 2 :value 1 :uid 1 :time 60}",  # stale: 2 was acknowledged at 40
    "{:type :ok :f :read :process 3 :value 2 :uid 2 :time 65}",
    "{:type :invoke :f :write :value 3 :process 0 :uid 3 :time 70}",
    "{:type :ok :f :write :process 0 :value 3 :uid 3 :time 80}",
    "{:type :invoke :f :read :value nil :process 1 :time 90}",
    "{:type :ok :f :read :process 1 :value 3 :uid 3 :time 100}",
])


def test_check_edn_catches_the_stale_read(validator):
    rep = J.check_edn(validator, STALE, realtime=True)
    assert rep["valid"] is True and rep["cycles"] == []
    assert rep["strict_valid"] is False
    assert rep["realtime_anomaly_types"] == ["G-single-realtime"]
    (c,) = rep["realtime_cycles"]
    ops = rep["history"].txn_ops
    assert sorted(c["txns"]) == [1, 2] and c["edge_types"] == ["rt", "rw"]
    assert c["ops"] == [ops[1], ops[2]]
    assert (ops[1][":f"], ops[1][":value"]) == (":write", 2) and (ops[2][":f"], ops[2][":value"]) == (":read", 1)
    assert rep["realtime_analysis"]["edges"] == 6
    # the default report is what it was
    plain = J.check_edn(validator, STALE)
    assert sorted(plain) == ["analysis", "anomaly_types", "cycles", "g2_keys", "history", "valid"]
    assert plain["valid"] is True
    # by line order too (no :time)
    import re
    assert J.check_edn(validator, re.sub(r" :time \d+", "", STALE), realtime=True)["strict_valid"] is False


def test_check_edn_reference_filetest_history(validator):
    golden = os.path.join(os.path.dirname(__file__), "golden", "jepsen_filetest_history.txt")
    rep = J.check_edn(validator, open(golden).read(), realtime=True)
    assert rep["valid"] is True and rep["strict_valid"] is True and rep["realtime_cycles"] == []


@pytest.mark.parametrize("seed", range(2))
def test_check_edn_register_histories(validator, oracle_mod, seed):
    # a serial execution logged at its commit times: linearizable by construction
    text, _ = J.register_history_edn(seed, n_ops=600, lost_update=0.0, stale_read=0.0)
    rep = J.check_edn(validator, text, realtime=True)
    assert rep["valid"] is True and rep["strict_valid"] is True
    assert rep["realtime_analysis"]["edges"] > 0
    # with injected lost updates and stale reads: against the CPU reference
    text, _ = J.register_history_edn(seed, n_ops=600)
    rep = J.check_edn(validator, text, realtime=True)
    assert rep["valid"] or not rep["strict_valid"]  # strict_valid => valid
    ops = rep["history"]
    h = ops.history
    edges = M.merged_edges(h.ntxn, oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed),
                           M.pairs(M.reduced(ops.invoke, ops.complete)) + (8,))
    ref = ref_anomalies(oracle_mod, h.ntxn, edges[0], edges[1], M.remap_types(edges[2]))
    res = rep["realtime_analysis"]
    assert res["edges"] == int(M.reduced(ops.invoke, ops.complete).sum())
    assert_matches(res, ref, h.ntxn)
    check_witnesses(dict(res, wit_type=M.remap_types(res["wit_type"]).astype(np.uint8)), ref)
    assert rep["strict_valid"] is False  # the injected stale reads
    plain_cls = rep["analysis"]["cls"]
    for c in rep["realtime_cycles"]:
        assert c["type"].endswith("-realtime") and not plain_cls[ref.scc == c["label"]].any()
    want = [int(l) for l in ref.comp_label if not plain_cls[ref.scc == l].any()]
    assert [c["label"] for c in rep["realtime_cycles"]] == want
    # stale reads alone: serializable, not strictly so, and every cycle needs real time
    text, _ = J.register_history_edn(seed, n_ops=600, lost_update=0.0)
    rep = J.check_edn(validator, text, realtime=True)
    assert rep["valid"] is True and rep["strict_valid"] is False
    assert rep["realtime_cycles"] and len(rep["realtime_cycles"]) == len(rep["realtime_analysis"]["comp_label"])
    assert all(t.endswith("-realtime") for t in rep["realtime_anomaly_types"])
    for c in rep["realtime_cycles"]:
        assert "rt" in "+".join(c["edge_types"])


def test_check_edn_adya_g2(validator):
    text, bad = J.adya_g2_edn(1, n_keys=300, anomaly=0.05)
    plain = J.check_edn(validator, text)
    rep = J.check_edn(validator, text, realtime=True)
    assert bad and rep["cycles"] == plain["cycles"] and rep["anomaly_types"] == plain["anomaly_types"] == ["G2"]
    assert rep["valid"] is False and rep["strict_valid"] is False
    scc, _ = validator.dep_graph_scc_built(rep["history"].history.ntxn)  # the real-time build's
    cls = rep["analysis"]["cls"]
    for c in rep["realtime_cycles"]:
        assert not cls[c["txns"]].any() and not cls[scc == c["label"]].any()
