"""The CPU side of the internal-consistency entries: the model of
internal_model.py against literal expectations, the pure report functions of
comdb2_amd/jepsen.py on model dicts, the host-only context, and the coverage of
the random generators for the seeds tests/test_gpu_internal.py runs."""
import copy

import numpy as np
import pytest

import internal_model as IM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J

N = IM.NONE


@pytest.mark.parametrize("name", sorted(IM.HAND))
def test_model_against_hand_literals(name):
    kind, h, want = IM.HAND[name]
    ref = IM.check(kind, h)
    IM.check_expected(ref, want)
    assert ref["nops"] == h.nops and ref["ntxn"] == h.ntxn
    assert ref["n_listed"] == ref["bad_reads"] == len(ref["listed_op"])
    if kind == "value":
        assert ref["compared_elements"] == 0
    # a write has no verdict; a bad read has an anchor
    for i in range(h.nops):
        if h.is_write[i]:
            assert ref["bad"][i] == 0 and ref["anchor_op"][i] == N
        if ref["bad"][i]:
            assert ref["anchor_op"][i] != N


def test_model_membership_is_the_resolves():
    """in_c decides what is counted, never what is flagged."""
    h = IM.HAND["v_write_read_different"][1]
    a, b = IM.check_values(h, in_c=[True]), IM.check_values(h, in_c=[False])
    assert a["bad"].tolist() == b["bad"].tolist() == [0, 1]
    assert (a["bad_reads"], b["bad_reads"], a["checked_reads"], b["checked_reads"]) == (1, 0, 1, 0)


def test_model_list_cap():
    ops = []
    for t in range(IM.LIST_CAP + 5):
        ops += [(t, 1, "w", t + 1), (t, 1, "r", None)]
    ref = IM.check_values(IM.vh(ops, [IM.OK] * (IM.LIST_CAP + 5)))
    assert ref["bad_reads"] == IM.LIST_CAP + 5 and ref["n_listed"] == IM.LIST_CAP
    assert ref["listed_op"].tolist() == [2 * t + 1 for t in range(IM.LIST_CAP)]
    assert ref["listed_anchor"].tolist() == [2 * t for t in range(IM.LIST_CAP)]


# ---- the report functions ------------------------------------------------------
BASE = {"valid": True, "anomaly_types": ["G1b"], "cycles": [],
        "levels": {"g1c_free": True, "read_committed": False, "snapshot_isolation": True, "serializable": True,
                   "strict_serializable": True, "strong_snapshot_isolation": False}}


def test_internal_reads_entries():
    kind, h, _ = IM.HAND["v_interleaved"]
    res = dict(IM.check(kind, h), ms=0.5, sort_packed=1)
    keys = J.internal_reads(h, res)
    assert keys["internal_anomaly_count"] == 2
    assert keys["internal_anomalies"] == [
        {"txn": 0, "key": 1, "op": 4, "anchor_op": 0, "expected": 1, "got": 2},
        {"txn": 1, "key": 1, "op": 6, "anchor_op": 3, "expected": 2, "got": 1}]
    assert keys["internal"]["bad_reads"] == 2 and keys["internal"]["ms"] == 0.5
    assert set(keys) == {"internal_anomalies", "internal_anomaly_count", "internal"}
    # the initial state reads as None on either side
    kind, h, _ = IM.HAND["v_init_after_own_write"]
    e, = J.internal_reads(h, IM.check(kind, h))["internal_anomalies"]
    assert (e["expected"], e["got"]) == (1, None)


def test_internal_list_reads_entries():
    kind, h, _ = IM.HAND["l_read_append_append_read_swapped"]
    keys = J.internal_list_reads(h, IM.check(kind, h))
    assert keys["internal_anomalies"] == [{"txn": 0, "key": 1, "op": 3, "anchor_op": 0, "prefix": [5],
                                           "appended": [10, 11], "got": [5, 11, 10]}]
    kind, h, _ = IM.HAND["l_append_append_read_wrong_suffix"]
    keys = J.internal_list_reads(h, IM.check(kind, h))
    assert keys["internal_anomalies"] == [{"txn": 0, "key": 1, "op": 2, "anchor_op": 0, "prefix": None,
                                           "appended": [10, 11], "got": [5, 11, 10]}]
    kind, h, _ = IM.HAND["l_append_read_append_read"]
    e, = J.internal_list_reads(h, IM.check(kind, h))["internal_anomalies"]
    assert (e["prefix"], e["appended"], e["got"]) == ([10], [11], [10, 12])
    assert J.internal_list_reads(h, IM.check(kind, h))["internal_anomaly_count"] == 1


def test_with_internal_ands_the_levels():
    kind, h, _ = IM.HAND["v_write_read_different"]
    before = copy.deepcopy(BASE)
    out = J.with_internal(BASE, J.internal_reads(h, IM.check(kind, h)))
    assert BASE == before  # a pure function
    assert out["valid"] is False and out["anomaly_types"] == ["G1b", "internal"]
    assert out["levels"] == {"g1c_free": True, "read_committed": False, "internal_consistent": False,
                             "snapshot_isolation": False, "serializable": False, "strict_serializable": False,
                             "strong_snapshot_isolation": False}
    assert out["internal_anomaly_count"] == 1 and len(out["internal_anomalies"]) == 1


def test_with_internal_clean_history_changes_no_verdict():
    kind, h, _ = IM.HAND["v_write_read_equal"]
    out = J.with_internal(BASE, J.internal_reads(h, IM.check(kind, h)))
    assert out["valid"] is True and out["anomaly_types"] == ["G1b"] and out["internal_anomalies"] == []
    assert out["levels"] == dict(BASE["levels"], internal_consistent=True)
    # without levels (no isolation) none appear; absent levels are not invented
    flat = {k: v for k, v in BASE.items() if k != "levels"}
    assert "levels" not in J.with_internal(flat, J.internal_reads(h, IM.check(kind, h)))
    few = dict(flat, levels={"g1c_free": True, "snapshot_isolation": True, "serializable": True})
    kind, h, _ = IM.HAND["v_write_read_different"]
    assert J.with_internal(few, J.internal_reads(h, IM.check(kind, h)))["levels"] == {
        "g1c_free": True, "snapshot_isolation": False, "serializable": False, "internal_consistent": False}


class _NoInternal:
    """A validator whose internal entries must not be reached."""

    def __getattr__(self, name):
        raise AssertionError(name)


def test_checks_default_to_no_internal_pass():
    """internal=False is the default of both checks: the first call either makes
    is the resolve, never an internal entry."""
    import inspect
    for f in (J.check_txn_edn, J.check_append_edn):
        assert inspect.signature(f).parameters["internal"].default is False
        with pytest.raises(AssertionError, match="resolve"):
            f(_NoInternal(), "{:type :ok :f :txn :value [[:r 1 nil]] :process 0}\n")


# ---- the host-only context -------------------------------------------------------
def test_host_only_context():
    v = hsc.Validator(-1)
    try:
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_internal -> -2:"):
            v.graph_internal()
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_internal_lists -> -2:"):
            v.graph_internal_lists(arrays=True)
    finally:
        v.close()


# ---- the generators keep exercising the path ---------------------------------------
@pytest.mark.parametrize("seed", IM.GPU_SEEDS)
def test_random_values_cover_the_path(seed):
    h = IM.random_values(seed)
    ref = IM.check_values(h)
    assert 15000 <= h.nops <= 25000
    assert ref["checked_reads"] >= 100 and 0 < ref["bad_reads"] < ref["checked_reads"]
    # txns are interleaved: some txn's ops are not contiguous
    t = np.asarray(h.txn)
    assert (np.diff(t) != 0).sum() > h.ntxn
    # flagged but uncounted reads exist (aborted / dropped txns)
    assert int(ref["bad"].sum()) > ref["bad_reads"]
    w = np.asarray(h.is_write) != 0
    pairs = set(zip(np.asarray(h.key)[w].tolist(), np.asarray(h.value)[w].tolist()))
    assert len(pairs) == int(w.sum())


@pytest.mark.parametrize("seed", IM.GPU_SEEDS)
def test_random_lists_cover_the_path(seed):
    h = IM.random_lists(seed)
    ref = IM.check_lists(h)
    assert 15000 <= h.nops <= 25000
    assert ref["checked_reads"] >= 100 and 0 < ref["bad_reads"] < ref["checked_reads"]
    assert ref["compared_elements"] > 0
    assert (np.diff(np.asarray(h.txn)) != 0).sum() > h.ntxn
    w = np.asarray(h.is_write) != 0
    pairs = set(zip(np.asarray(h.key)[w].tolist(), np.asarray(h.value)[w].tolist()))
    assert len(pairs) == int(w.sum())
    # the resolve's model accepts the history (no duplicated append, offsets ascending)
    import lists_model as LM
    LM.resolve(h)


def test_random_full_width_keys():
    for h in (IM.random_values(5, n_txn=200, full64=True), IM.random_lists(5, n_txn=200, full64=True)):
        assert int(np.asarray(h.key).max()) > 2 ** 60
