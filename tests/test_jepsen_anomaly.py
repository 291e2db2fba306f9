"""Jepsen histories -> which anomaly, and the ops to look at:
jepsen.anomaly_report (a pure function, CPU) and jepsen.check_edn (-m gpu),
against the reference of tests/test_anomaly.py."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

from comdb2_amd import jepsen as J
from test_anomaly import check_witnesses, ref_of_history


def _g2_result(ops, keys):
    """What dep_graph_anomalies returns for an adya history whose ``keys``
    have two :ok inserts: per key the 2-cycle of rw edges between them."""
    by_key = {}
    for t, op in enumerate(ops.txn_ops):
        by_key.setdefault(int(op[":value"][0]), []).append(t)
    pairs = sorted((max(by_key[k]), min(by_key[k])) for k in keys)
    cls = np.zeros(ops.history.ntxn, np.uint8)
    for hi, lo in pairs:
        cls[[hi, lo]] = 4
    n = len(pairs)
    return {"cls": cls, "comp_label": np.array([p[0] for p in pairs], np.uint32),
            "comp_class": np.full(n, 4, np.uint8), "wit_off": np.arange(n + 1, dtype=np.uint32) * 2,
            "wit_txn": np.array([t for hi, lo in pairs for t in (hi, lo)], np.uint32),
            "wit_type": np.full(2 * n, 4, np.uint8)}


def test_report_names_the_g2_inserts():
    text, bad = J.adya_g2_edn(5, n_keys=120, anomaly=0.1)
    assert bad
    ops = J.history_from_jepsen_edn(text)
    rep = J.anomaly_report(ops, _g2_result(ops, bad))
    assert not rep["valid"] and rep["anomaly_types"] == ["G2"]
    assert sorted(rep["g2_keys"]) == sorted(bad)
    assert len(rep["cycles"]) == len(bad)
    seen = []
    for cyc in rep["cycles"]:
        assert cyc["type"] == "G2" and cyc["edge_types"] == ["rw", "rw"] and len(cyc["txns"]) == 2
        assert cyc["label"] == max(cyc["txns"])
        assert all(op[":type"] == ":ok" and op[":f"] == ":insert" for op in cyc["ops"])
        keys = {int(op[":value"][0]) for op in cyc["ops"]}
        assert len(keys) == 1
        # one insert into table a, one into table b
        assert sorted(op[":value"][1][0] is None for op in cyc["ops"]) == [False, True]
        seen += keys
    assert sorted(seen) == sorted(bad)


def test_report_of_a_register_history_with_a_made_up_witness():
    text, _ = J.register_history_edn(2, n_ops=200)
    ops = J.history_from_jepsen_edn(text)
    assert ops.history.ntxn > 12
    result = {"cls": np.zeros(ops.history.ntxn, np.uint8), "comp_label": np.array([7, 12], np.uint32),
              "comp_class": np.array([2, 1], np.uint8), "wit_off": np.array([0, 3, 5], np.uint32),
              "wit_txn": np.array([3, 7, 5, 12, 10], np.uint32),
              "wit_type": np.array([2, 1, 4, 6, 3], np.uint8)}
    rep = J.anomaly_report(ops, result)
    assert not rep["valid"] and rep["anomaly_types"] == ["G-single", "G1c"] and rep["g2_keys"] == {}
    a, b = rep["cycles"]
    assert (a["type"], a["label"], a["txns"], a["edge_types"]) == ("G-single", 7, [3, 7, 5], ["wr", "ww", "rw"])
    assert a["ops"] == [ops.txn_ops[3], ops.txn_ops[7], ops.txn_ops[5]]
    assert (b["type"], b["txns"], b["edge_types"]) == ("G1c", [12, 10], ["wr+rw", "ww+wr"])
    # without witnesses: the classes alone
    bare = dict(result, wit_off=np.zeros(3, np.uint32), wit_txn=np.zeros(0, np.uint32),
                wit_type=np.zeros(0, np.uint8))
    rep = J.anomaly_report(ops, bare)
    assert [c["type"] for c in rep["cycles"]] == ["G-single", "G1c"]
    assert all(c["txns"] == [] and c["ops"] == [] for c in rep["cycles"])


def test_report_of_no_cycle_is_valid():
    text, _ = J.register_history_edn(1, n_ops=50, lost_update=0.0, stale_read=0.0)
    ops = J.history_from_jepsen_edn(text)
    for result in ({}, {"cls": np.zeros(ops.history.ntxn, np.uint8), "comp_label": np.zeros(0, np.uint32),
                        "comp_class": np.zeros(0, np.uint8), "wit_off": np.zeros(1, np.uint32),
                        "wit_txn": np.zeros(0, np.uint32), "wit_type": np.zeros(0, np.uint8)}):
        rep = J.anomaly_report(ops, result)
        assert rep == {"valid": True, "anomaly_types": [], "cycles": [], "g2_keys": {}}


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [0, 1])
def test_gpu_check_edn_adya_g2(validator, oracle_mod, seed):
    text, bad = J.adya_g2_edn(seed, n_keys=200, anomaly=0.1)
    assert bad
    rep = J.check_edn(validator, text)
    assert not rep["valid"] and rep["anomaly_types"] == ["G2"]
    assert all(c["type"] == "G2" and c["edge_types"] == ["rw", "rw"] for c in rep["cycles"])
    keys = [{int(op[":value"][0]) for op in c["ops"]} for c in rep["cycles"]]
    assert all(len(k) == 1 for k in keys)
    assert sorted(k for ks in keys for k in ks) == sorted(bad) == sorted(rep["g2_keys"])
    ref = ref_of_history(oracle_mod, rep["history"].history)
    np.testing.assert_array_equal(rep["analysis"]["cls"], ref.cls)
    check_witnesses(rep["analysis"], ref)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_keys", [(0, 1), (1, 1), (2, 3)])
def test_gpu_check_edn_register(validator, oracle_mod, seed, n_keys):
    text, _ = J.register_history_edn(seed, n_ops=1500, n_keys=n_keys)
    rep = J.check_edn(validator, text)
    h = rep["history"].history
    ref = ref_of_history(oracle_mod, h)
    res = rep["analysis"]
    np.testing.assert_array_equal(res["cls"], ref.cls)
    np.testing.assert_array_equal(res["comp_label"], ref.comp_label)
    np.testing.assert_array_equal(res["comp_class"], ref.comp_class)
    assert res["anti_edges"] == res["anti_tested"] == ref.anti_edges
    check_witnesses(res, ref)
    assert rep["valid"] == (len(ref.comp_label) == 0)
    assert rep["anomaly_types"] == sorted({J.ANOMALY_NAMES[int(k)] for k in ref.comp_class})
    assert [c["label"] for c in rep["cycles"]] == ref.comp_label.tolist()
    for c in rep["cycles"]:
        assert c["ops"] == [rep["history"].txn_ops[t] for t in c["txns"]]
    bare = J.check_edn(validator, text, witness=False)
    assert bare["anomaly_types"] == rep["anomaly_types"] and all(c["txns"] == [] for c in bare["cycles"])
