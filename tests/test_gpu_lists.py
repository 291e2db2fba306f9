"""hsc_dep_graph_resolve_lists / _build_lists on the GPU (include/hip_serial.h,
DESIGN.md §5h): every counter and array must equal the CPU reference of
lists_model.py exactly, the edges of the build must equal the reference's
merged edge set, and the classes of the anomaly and snapshot-isolation entries
on that build must equal the existing CPU references over that edge set."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import lists_model as M
import realtime_model as R
from comdb2_amd import hsc
from comdb2_amd import jepsen as J
from comdb2_amd.workloads import config4_history
from si_model import ref_si
from test_anomaly import ref_anomalies

pytestmark = pytest.mark.gpu

OK, ABORTED, UNKNOWN = M.OK, M.ABORTED, M.UNKNOWN
SCAN_TILE = 2048  # scan_exclusive_u32: 256 threads x 8 items per workgroup


def edges_of(validator):
    return [a.copy() for a in validator.dep_graph_edges()]


def run(validator, h, arrays=True, ref=None, oracle_mod=None):
    """Resolve + build on the GPU against the model: counters, arrays, edges,
    and (with the oracle) the classes of the components."""
    ref = M.resolve(h) if ref is None else ref
    res = validator.graph_resolve_lists(h, arrays=arrays)
    M.assert_equal(res, ref, arrays=arrays)
    st = validator.graph_build_lists(full=True)
    got = edges_of(validator)
    for a, b in zip(got, ref["edges"]):
        np.testing.assert_array_equal(a, b)
    t = ref["edges"][2]
    assert [st[k] for k in ("edges", "ww", "wr", "rw")] == [len(t)] + [int((t & b != 0).sum()) for b in (1, 2, 4)]
    if oracle_mod is not None:
        s, d, t = ref["edges"]
        an, si = validator.dep_graph_anomalies(), validator.dep_graph_si()
        want = ref_anomalies(oracle_mod, ref["ncommitted"], s, d, t)
        for k in ("cls", "comp_label", "comp_class"):
            np.testing.assert_array_equal(an[k], getattr(want, k), err_msg=k)
        want_si = ref_si(oracle_mod, ref["ncommitted"], s, d, t)
        for k in ("nonadj", "comp_label", "comp_nonadj"):
            np.testing.assert_array_equal(si[k], getattr(want_si, k), err_msg=k)
    return res, ref


# ---- hand-built cases ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.HAND))
def test_hand_built(validator, oracle_mod, name):
    h, want = M.HAND[name]
    res, ref = run(validator, h, oracle_mod=oracle_mod)
    M.check_expected(dict(res, edges=ref["edges"]), want)
    bare, _ = run(validator, h, arrays=False)
    M.check_expected(dict(bare, edges=ref["edges"]), {k: v for k, v in want.items() if k not in M.OP_ARRAYS})


# ---- state and errors -----------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.INVALID))
def test_invalid_history(validator, name):
    with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_resolve_lists -> -1:"):
        validator.graph_resolve_lists(M.INVALID[name])
    # a failed resolve leaves nothing to build
    with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_build_lists -> -5:"):
        validator.graph_build_lists()
    run(validator, M.HAND["g1b"][0])  # and the context goes on working


def test_host_only_context_and_state():
    v = hsc.Validator(-1)
    try:
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_resolve_lists -> -2:"):
            v.graph_resolve_lists(M.HAND["g1a"][0])
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_build_lists -> -2:"):
            v.graph_build_lists()
    finally:
        v.close()


def test_build_lists_before_any_resolve():
    v = hsc.Validator(0)
    try:
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_build_lists -> -5:"):
            v.graph_build_lists()
    finally:
        v.close()


def test_empty_history(validator):
    res, _ = run(validator, M.lh([], []))
    assert res["ncommitted"] == 0 and res["keys"] == 0 and res["elements"] == 0
    # txns without ops
    res, _ = run(validator, M.lh([], [OK, ABORTED, UNKNOWN]))
    assert res["fate"].tolist() == [0, 1, 2] and res["ncommitted"] == 1
    # appends nobody read: no spine, no rows
    res, _ = run(validator, M.lh([(0, 1, 10), (1, 1, 11)], [OK, OK]))
    assert res["unobserved_appends"] == 2 and res["spine_elements"] == 0


def test_staged_rw_pairs_are_refused_and_kept():
    from comdb2_amd.workloads import history_window, int64_words
    h = config4_history(n_txn=300, n_keys=40, concurrent_frac=0.3, max_lag=16)
    hw = history_window(h)
    ids = np.arange(h.ntxn)
    lists, ref = M.HAND["g0"][0], M.resolve(M.HAND["g0"][0])
    v = hsc.Validator(0)
    try:
        v.register_group("t1", 0, 9)
        dev = torch.device("cuda", 0)
        gid = torch.zeros(len(hw.keys), dtype=torch.int32, device=dev)
        words = torch.from_numpy(int64_words(hw.keys).reshape(-1).view(np.int64)).to(dev)
        lsn = torch.from_numpy(hw.lsn.view(np.int64)).to(dev)
        v.ingest_device(len(hw.keys), 2, gid.data_ptr(), words.data_ptr(), lsn.data_ptr(), hw.end_lsn)
        torch.cuda.synchronize()
        assert len(v.rw_edges(hw.readsets)[0]) > 0
        v.dep_graph_stage_rw_pairs(ids, hw.commit_lsn, ids)
        v.graph_resolve_lists(lists)
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_build_lists -> -1:"):
            v.graph_build_lists()
        # still staged: a build without rw edges of its own gets them from the pairs
        st = v.dep_graph_build(h, full=True, no_rw=True)
        assert st["rw"] > 0
        # and now the list build goes through, from the resolve made before
        v.graph_build_lists()
        for a, b in zip(edges_of(v), ref["edges"]):
            np.testing.assert_array_equal(a, b)
    finally:
        v.close()


def test_plain_build_between_resolve_and_its_build(validator):
    h, ref = M.gen_case("seed11")
    other = config4_history(seed=8, n_txn=700, n_keys=500)
    validator.graph_resolve_lists(h, arrays=False)
    validator.dep_graph_build(other, full=True)
    want_other = edges_of(validator)
    validator.graph_build_lists(full=True)
    for a, b in zip(edges_of(validator), ref["edges"]):
        np.testing.assert_array_equal(a, b)
    # and the other way: the list resolve does not disturb a plain build's edges
    validator.dep_graph_build(other, full=True)
    validator.graph_resolve_lists(h, arrays=False)
    for a, b in zip(edges_of(validator), want_other):
        np.testing.assert_array_equal(a, b)


def test_staged_realtime_order_joins(validator):
    h, ref = M.gen_case("full64")
    nc = ref["ncommitted"]
    invoke, complete = R.random_intervals(5, nc, procs=6)
    validator.graph_resolve_lists(h, arrays=False)
    staged = validator.dep_graph_stage_realtime(invoke, complete)
    assert staged["edges"] > 0
    validator.graph_build_lists(full=True)
    rs, rd = R.reduced_sorted(invoke, complete)
    want = R.merged_edges(nc, tuple(a.astype(np.int64) for a in ref["edges"]),
                          (rs, rd, np.full(len(rs), 8, np.int64)))
    for a, b in zip(edges_of(validator), want):
        np.testing.assert_array_equal(a, b)
    # the order joined once: the next build is the plain one
    validator.graph_build_lists(full=True)
    for a, b in zip(edges_of(validator), ref["edges"]):
        np.testing.assert_array_equal(a, b)


# ---- shapes -------------------------------------------------------------------
def one_key(length, reads, key=5, writers=3, status=None, extra=()):
    """``writers`` txns append ``length`` elements to one key in turn; txn
    ``writers`` reads the whole list, and one more txn per entry of ``reads``
    reads that prefix (an int) or that list."""
    elems = [100 + i for i in range(length)]
    ops = [(i % writers, key, e) for i, e in enumerate(elems)]
    ops.append((writers, key, elems))
    for j, r in enumerate(reads):
        ops.append((writers + 1 + j, key, elems[:r] if isinstance(r, int) else r))
    ops += list(extra)
    nt = max(t for t, _, _ in ops) + 1
    return M.lh(ops, status or [OK] * nt)


@pytest.mark.parametrize("length", [255, 256, 257])
def test_spine_length_at_the_workgroup(validator, length):
    res, _ = run(validator, one_key(length, [0, 1, length - 1, length]))
    assert res["spine_elements"] == length and res["chain_entries"] == length and res["ww"] == length - 1


@pytest.mark.parametrize("length", [SCAN_TILE - 2, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1])
def test_spine_length_at_the_scan_block(validator, length):
    # the spine's scans run over length + 1 words
    res, _ = run(validator, one_key(length, [length - 1, SCAN_TILE - 3, 7]))
    assert res["spine_elements"] == length and res["wr"] == 4 and res["rw"] == 3


def test_read_straddling_two_compare_workgroups(validator):
    # the spine takes elements [0, 200), the next read [200, 300): it crosses element 256
    elems = [100 + i for i in range(200)]
    bad = elems[:100]
    bad[70] = 7  # position 270 of the element array
    res, _ = run(validator, one_key(200, [100, bad]))
    # (the prefix of 100 ends at an append that is not its writer's last: intermediate)
    assert res["rflag"].tolist()[-2:] == [M.B, M.X]


@pytest.mark.parametrize("at", [0, 63, 64, 65, 129])
def test_first_mismatch_position(validator, at):
    elems = [100 + i for i in range(130)]
    bad = list(elems)
    bad[at] = 9
    res, _ = run(validator, one_key(130, [130, bad, 129]))
    assert res["rflag"].tolist()[-3:] == [0, M.X, 0] and res["incompatible_keys"] == 1


def test_one_hot_key_holds_every_op(validator, oracle_mod):
    length = 3000
    reads = list(range(0, length, 17)) + [[100, 102]]
    status = [OK, ABORTED, UNKNOWN] + [OK] * (1 + len(reads))
    res, ref = run(validator, one_key(length, reads, status=status), oracle_mod=oracle_mod)
    assert res["keys"] == 1 and res["g1a_reads"] > 100 and res["recovered"] == 1 and res["incompatible_reads"] == 1


def test_extreme_keys(validator):
    ops = []
    for q, k in enumerate([0, 1, 2 ** 63, 2 ** 64 - 2]):
        ops += [(0, k, 10 + q), (1, k, 20 + q), (2, k, [10 + q, 20 + q]), (3, k, [10 + q])]
    ops += [(3, 2 ** 64 - 3, [])]  # a key nobody appended to
    res, _ = run(validator, M.lh(ops, [OK] * 4))
    assert res["keys"] == 5 and res["spine_op"].tolist() == [2, 6, 10, 16, 14]


def test_reads_tied_for_longest(validator):
    elems = [100 + i for i in range(70)]
    res, _ = run(validator, one_key(70, [70, 70, 69, elems[:69] + [5]]))
    assert res["spine_op"].tolist() == [70] and res["incompatible_reads"] == 1


@pytest.mark.parametrize("k", [hsc.RESOLVE_LIST_CAP - 1, hsc.RESOLVE_LIST_CAP, hsc.RESOLVE_LIST_CAP + 1])
def test_listed_cap(validator, k):
    # an aborted txn's element in the list: every read of it is a G1a read
    ops = [(0, 3, 1)] + [(1, 3, [1])] * k
    res, ref = run(validator, M.lh(ops, [ABORTED, OK]))
    assert res["g1a_reads"] == k and res["n_listed"] == min(k, hsc.RESOLVE_LIST_CAP)
    assert ref["n_listed_exact"] == k and len(res["listed_op"]) == res["n_listed"]


@pytest.mark.parametrize("name", ["seed11", "seed12"])
@pytest.mark.parametrize("arrays", [True, False])
def test_generated(validator, oracle_mod, name, arrays):
    h, ref = M.gen_case(name)
    res, _ = run(validator, h, arrays=arrays, ref=ref, oracle_mod=oracle_mod if arrays else None)
    assert h.ntxn > 4000 and res["g1a_reads"] > 0 and res["incompatible_reads"] > 0


def test_full_64_bit_keys_and_elements(validator, oracle_mod):
    # the whole-row sorts (seed11 / seed12 sort packed)
    h, ref = M.gen_case("full64")
    run(validator, h, ref=ref, oracle_mod=oracle_mod)


# ---- Jepsen ---------------------------------------------------------------------------
# Two writers of key 1: the database applied txn B's append after txn A's --
# B read A's append of key 2 -- but B's completion came back first.
APPEND_REORDERED = """
{:type :invoke :f :txn :value [[:append 1 1] [:append 2 1]] :process 0 :time 1}
{:type :invoke :f :txn :value [[:r 2 nil] [:append 1 2]] :process 1 :time 2}
{:type :ok :f :txn :value [[:r 2 [1]] [:append 1 2]] :process 1 :time 3}
{:type :ok :f :txn :value [[:append 1 1] [:append 2 1]] :process 0 :time 4}
{:type :invoke :f :txn :value [[:r 1 nil]] :process 2 :time 5}
{:type :ok :f :txn :value [[:r 1 [1 2]]] :process 2 :time 6}
"""
# the same schedule as an rw-register history
REGISTER_REORDERED = """
{:type :invoke :f :txn :value [[:w 1 1] [:w 2 1]] :process 0 :time 1}
{:type :invoke :f :txn :value [[:r 2 nil] [:w 1 2]] :process 1 :time 2}
{:type :ok :f :txn :value [[:r 2 1] [:w 1 2]] :process 1 :time 3}
{:type :ok :f :txn :value [[:w 1 1] [:w 2 1]] :process 0 :time 4}
{:type :invoke :f :txn :value [[:r 1 nil]] :process 2 :time 5}
{:type :ok :f :txn :value [[:r 1 2]] :process 2 :time 6}
"""


def test_completion_order_against_version_order(validator):
    """Why the entry exists: a serializable history whose two writers of one
    key complete in the opposite order to their version order is valid as a
    list-append history, while the rw-register check, which must take
    completion order for version order, reports a cycle on the same schedule."""
    rep = J.check_append_edn(validator, APPEND_REORDERED, realtime=True, isolation=True)
    assert rep["valid"] is True and rep["cycles"] == [] and rep["anomaly_types"] == []
    assert rep["strict_valid"] is True and rep["levels"]["serializable"] is True
    assert rep["resolve"]["ww"] == 1 and rep["resolve"]["wr"] == 2
    reg = J.check_txn_edn(validator, REGISTER_REORDERED)
    assert reg["valid"] is False and [c["type"] for c in reg["cycles"]] == ["G1c"]
    assert sorted(reg["cycles"][0]["txns"]) == [0, 1]


def model_report(oracle_mod, text):
    """check_append_edn's verdicts assembled from the CPU references."""
    tx = J.lhistory_from_append_edn(text)
    ref = M.resolve(tx.lhistory)
    s, d, t = ref["edges"]
    an = ref_anomalies(oracle_mod, ref["ncommitted"], s, d, t)
    si = ref_si(oracle_mod, ref["ncommitted"], s, d, t)
    toc = ref["txn_of_cid"].tolist()
    types = {J.ANOMALY_NAMES[int(k)] for k in an.comp_class}
    for name, k in (("G1a", "g1a_reads"), ("G1b", "g1b_reads"), ("incompatible-order", "incompatible_reads"),
                    ("duplicate-elements", "duplicate_reads")):
        if ref[k]:
            types.add(name)
    g1 = ref["g1a_reads"] > 0 or ref["g1b_reads"] > 0
    out = {"ref": ref, "types": types, "valid": not types,
           "cycles": [{"type": J.ANOMALY_NAMES[int(k)], "label": toc[int(l)]}
                      for l, k in zip(an.comp_label, an.comp_class)],
           "si_cycles": [{"type": "G-nonadjacent" if int(k) == 4 else J.ANOMALY_NAMES[int(k)], "label": toc[int(l)]}
                         for l, k, f in zip(an.comp_label, an.comp_class, si.comp_nonadj) if f],
           "levels": {"g1c_free": not (an.cls & 1).any(), "snapshot_isolation": not si.comp_nonadj.any(),
                      "serializable": len(an.comp_label) == 0}}
    out["levels"]["read_committed"] = not g1 and out["levels"]["g1c_free"]
    out["listed"] = J.listed_list_reads(tx.lhistory, ref)
    return out


def assert_report(validator, oracle_mod, text, **kw):
    got = J.check_append_edn(validator, text, isolation=True, **kw)
    want = model_report(oracle_mod, text)
    assert set(got["anomaly_types"]) - {"G0"} == want["types"]
    assert got["valid"] == (want["valid"] and "G0" not in got["anomaly_types"])
    for k in ("cycles", "si_cycles"):
        assert [{q: c[q] for q in ("type", "label")} for c in got[k]] == want[k], k
        for c in got[k]:
            assert len(c["txns"]) == len(c["edge_types"]) == len(c["ops"]) >= 2
    assert {k: got["levels"][k] for k in want["levels"]} == want["levels"]
    for k, v in want["listed"].items():
        assert got[k] == v, k
    for k in M.COUNTS:
        assert got["resolve"][k] == want["ref"][k], k
    for k in ("fate", "cid", "txn_of_cid", "txn_g1"):
        np.testing.assert_array_equal(got["resolve_arrays"][k], want["ref"][k])
    return got


@pytest.mark.parametrize("seed", [1, 2])
def test_check_append_edn_with_injections(validator, oracle_mod, seed):
    text, inj = J.append_history_edn(seed, n_txns=1500, n_keys=40)
    assert all(v > 0 for v in inj.values()), inj
    rep = assert_report(validator, oracle_mod, text)
    assert rep["valid"] is False
    assert {"G0", "G1a", "G1b", "G1c", "G-single", "G2", "incompatible-order", "duplicate-elements"} <= \
        set(rep["anomaly_types"])
    assert rep["duplicate_read_count"] > 0 and rep["incompatible_reads"] and rep["duplicate_reads"]
    # the G0 gadget's component holds ww edges only between its two writers
    assert any(c["g0"] and len(c["txns"]) == 2 for c in rep["cycles"])


def test_check_append_edn_clean(validator, oracle_mod):
    text, _ = J.append_history_edn(3, n_txns=1500, n_keys=40, dirty=0, intermediate=0, dangling=0, duplicate=0,
                                   incompatible=0, cycles=False)
    rep = assert_report(validator, oracle_mod, text, realtime=True)
    assert rep["valid"] is True and rep["strict_valid"] is True and rep["anomaly_types"] == []
    assert rep["levels"] == {"g1c_free": True, "snapshot_isolation": True, "serializable": True,
                             "read_committed": True, "strict_serializable": True, "strong_snapshot_isolation": True}
    assert rep["resolve"]["recovered"] > 0 and rep["resolve"]["ww"] > 500
    # the premise the rw-register check needs does not hold here: the version
    # orders the reads give go against completion order (= txn id) many times
    tx = rep["history"]
    s, d, t = validator.dep_graph_edges()
    toc = rep["resolve_arrays"]["txn_of_cid"]
    done = tx.complete[toc]
    ww = ((t & 1) != 0) & (done[s] != J.RT_OPEN) & (done[d] != J.RT_OPEN)
    assert (done[s[ww]] > done[d[ww]]).sum() > 10
