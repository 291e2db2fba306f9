"""jepsen.vhistory_from_txn_edn / dirty_reads_from_edn on hand-written EDN, and
check_txn_edn / check_dirty_reads_edn with a stub validator whose resolve is
the CPU reference (resolve_model.py)."""
import numpy as np

import resolve_model as M
from comdb2_amd import jepsen as J

RT_OPEN = J.RT_OPEN

# p0 fails a write of x = 1 that p1 then reads; p2 crashes (:info) after a write p1 reads later; p3's
# invoke never completes and nobody sees its write
TXNS = """
{:type :invoke :f :txn :value [[:w 1 1] [:w 2 5]] :process 0 :time 10}
{:type :invoke :f :txn :value [[:r 1 nil] [:r 9 nil]] :process 1 :time 11}
{:type :fail :f :txn :value [[:w 1 1] [:w 2 5]] :process 0 :time 20}
{:type :ok :f :txn :value [[:r 1 1] [:r 9 nil]] :process 1 :time 30}
{:type :invoke :f :txn :value [[:r 2 nil] [:w 2 6] [:w 2 7]] :process 2 :time 35}
{:type :invoke :f :txn :value [[:w 3 8]] :process 3 :time 36}
{:type :info :f :txn :value [[:r 2 nil] [:w 2 6] [:w 2 7]] :process 2 :time 40}
{:type :invoke :f :txn :value [[:r 2 nil] [:w 4 9]] :process 1 :time 50}
{:type :ok :f :txn :value [[:r 2 6] [:w 4 9]] :process 1 :time 60}
"""


def test_vhistory_from_txn_edn():
    tx = J.vhistory_from_txn_edn(TXNS)
    v = tx.vhistory
    # ids: fail@20, ok@30, info by its invoke@35, unpaired by its invoke@36, ok@60
    assert (tx.ok, tx.failed, tx.info, tx.unpaired) == (2, 1, 1, 1)
    assert v.status.tolist() == [M.ABORTED, M.OK, M.UNKNOWN, M.UNKNOWN, M.OK] and v.ntxn == 5
    assert v.txn.tolist() == [0, 0, 1, 1, 2, 2, 3, 4, 4]
    assert v.key.tolist() == [1, 2, 1, 9, 2, 2, 3, 2, 4]
    assert v.is_write.tolist() == [1, 1, 0, 0, 1, 1, 1, 0, 1]
    assert v.value.tolist() == [1, 5, 1, M.INIT, 6, 7, 8, 6, 9]  # the :info op's read is left out
    assert tx.invoke.tolist() == [10, 11, 35, 36, 50]
    assert tx.complete.tolist() == [20, 30, RT_OPEN, RT_OPEN, 60]
    assert [o[":type"] for o in tx.txn_ops] == [":fail", ":ok", ":info", ":invoke", ":ok"]
    res = M.resolve(v)
    assert res["fate"].tolist() == [1, 0, 3, 2, 0]
    assert (res["g1a_reads"], res["g1b_reads"]) == (1, 1)


def test_vhistory_without_times_uses_lines():
    text = TXNS
    import re
    tx = J.vhistory_from_txn_edn(re.sub(r" :time \d+", "", text))
    assert tx.vhistory.status.tolist() == [M.ABORTED, M.OK, M.UNKNOWN, M.UNKNOWN, M.OK]
    assert tx.invoke.tolist() == [0, 1, 4, 5, 7] and tx.complete.tolist() == [2, 3, RT_OPEN, RT_OPEN, 8]


class Stub:
    """resolve = the CPU reference; the graph analyses find what they are given."""

    def __init__(self, anomalies=None, si=None):
        self.calls, self.anomalies, self.si = [], anomalies, si

    def dep_graph_resolve(self, vh, arrays=True):
        self.calls.append(("resolve", arrays))
        self.res = dict(M.resolve(vh), sweeps=4, ms=0.5)
        return self.res

    def dep_graph_build_resolved(self, full=True, no_rw=False):
        self.calls.append(("build_resolved", full))
        return {}

    def dep_graph_anomalies(self, witness=True, max_anti_batches=0):
        self.calls.append(("anomalies", witness))
        n = self.res["ncommitted"]
        return self.anomalies or {"cls": np.zeros(n, np.uint8), "comp_label": np.zeros(0, np.uint32),
                                  "comp_class": np.zeros(0, np.uint8), "wit_off": np.zeros(1, np.uint32),
                                  "wit_txn": np.zeros(0, np.uint32), "wit_type": np.zeros(0, np.uint8),
                                  "comps": [0, 0, 0], "txns": [0, 0, 0]}

    def dep_graph_si(self, witness=True):
        self.calls.append(("si", witness))
        return self.si or {"comp_label": np.zeros(0, np.uint32), "comp_nonadj": np.zeros(0, np.uint8),
                           "wit_off": np.zeros(1, np.uint32), "wit_txn": np.zeros(0, np.uint32),
                           "wit_type": np.zeros(0, np.uint8)}

    def dep_graph_stage_realtime(self, invoke, complete):
        self.calls.append(("stage", np.asarray(invoke).tolist(), np.asarray(complete).tolist()))
        return {"edges": 1, "ms": 0.25}

    def dep_graph_scc_built(self, ntxn):
        self.calls.append(("scc", ntxn))
        return np.arange(ntxn, dtype=np.uint32), {}


def test_check_txn_edn_reports_g1a_and_g1b_without_a_cycle():
    s = Stub()
    rep = J.check_txn_edn(s, TXNS, isolation=True)
    assert [c[0] for c in s.calls] == ["resolve", "build_resolved", "anomalies", "si"]
    assert rep["valid"] is False and rep["cycles"] == []
    assert rep["anomaly_types"] == ["G1a", "G1b"]
    assert rep["levels"]["read_committed"] is False and rep["levels"]["serializable"] is True
    assert rep["aborted_reads"] == [{"reader": 1, "writer": 0, "key": 1, "value": 1, "reader_op": 2, "writer_op": 0}]
    assert rep["intermediate_reads"] == [{"reader": 4, "writer": 2, "key": 2, "value": 6, "reader_op": 7,
                                          "writer_op": 4}]
    assert rep["dangling_reads"] == []
    assert (rep["aborted_read_count"], rep["intermediate_read_count"], rep["dangling_read_count"]) == (1, 1, 0)
    assert rep["resolve"]["recovered"] == 1 and rep["resolve"]["dropped"] == 1 and rep["resolve"]["sweeps"] == 4
    assert rep["history"].vhistory.ntxn == 5


def test_check_txn_edn_maps_cycles_back_and_stages_committed_intervals():
    # committed ids: 0 = txn 1, 1 = txn 2 (recovered), 2 = txn 4
    an = {"cls": np.array([4, 0, 4], np.uint8), "comp_label": np.array([2], np.uint32),
          "comp_class": np.array([4], np.uint8), "wit_off": np.array([0, 2], np.uint32),
          "wit_txn": np.array([0, 2], np.uint32), "wit_type": np.array([4, 4], np.uint8),
          "comps": [0, 0, 1], "txns": [0, 0, 2]}
    s = Stub(an)
    rep = J.check_txn_edn(s, TXNS, realtime=True)
    assert [c[0] for c in s.calls] == ["resolve", "build_resolved", "anomalies", "stage", "build_resolved",
                                       "anomalies", "scc"]
    assert s.calls[3] == ("stage", [11, 35, 50], [30, RT_OPEN, 60])  # the recovered txn is open
    assert s.calls[-1] == ("scc", 3)
    (c,) = rep["cycles"]
    assert c["txns"] == [1, 4] and c["label"] == 4 and c["type"] == "G2"
    assert [o[":time"] for o in c["ops"]] == [30, 60]
    assert rep["anomaly_types"] == ["G1a", "G1b", "G2"] and rep["valid"] is False
    assert rep["resolve_arrays"]["txn_of_cid"].tolist() == [1, 2, 4]


def test_check_txn_edn_clean_history_is_valid_and_read_committed():
    text = """
{:type :invoke :f :txn :value [[:w 1 1]] :process 0 :time 1}
{:type :ok :f :txn :value [[:w 1 1]] :process 0 :time 2}
{:type :invoke :f :txn :value [[:r 1 nil]] :process 1 :time 3}
{:type :ok :f :txn :value [[:r 1 1]] :process 1 :time 4}
"""
    rep = J.check_txn_edn(Stub(), text, isolation=True)
    assert rep["valid"] is True and rep["anomaly_types"] == []
    assert rep["levels"]["read_committed"] is True


DIRTY = """
{:type :invoke :f :write :value 1 :process 0 :time 1}
{:type :ok :f :write :value 1 :process 0 :time 2}
{:type :invoke :f :write :value 2 :process 1 :time 3}
{:type :fail :f :write :value 2 :process 1 :time 4 :reason "x"}
{:type :invoke :f :read :value nil :process 2 :time 5}
{:type :ok :f :read :value [1 1 1] :process 2 :time 6}
{:type :invoke :f :read :value nil :process 2 :time 7}
{:type :ok :f :read :value [1 2 1] :process 2 :time 8}
{:type :invoke :f :read :value nil :process 3 :time 9}
{:type :ok :f :read :value [2] :process 3 :time 10}
{:type :invoke :f :write :value 3 :process 0 :time 11}
{:type :ok :f :write :value 3 :process 0 :time 12}
{:type :invoke :f :read :value nil :process 3 :time 13}
{:type :ok :f :read :value [3 1] :process 3 :time 14}
{:type :invoke :f :read :value nil :process 4 :time 15}
{:type :fail :f :read :value nil :process 4 :time 16}
"""


def test_dirty_reads_from_edn():
    d = J.dirty_reads_from_edn(DIRTY)
    v = d.ops.vhistory
    assert d.n == 3 and d.short_reads == 2 and d.reads == [2, 3, 4, 6]
    assert v.status.tolist() == [0, 1, 0, 0, 0, 0, 0, 1]
    assert v.txn.tolist() == [0] * 3 + [1] * 3 + [2] * 3 + [3] * 3 + [4] + [5] * 3 + [6] * 2
    assert v.key.tolist() == [0, 1, 2] * 4 + [0] + [0, 1, 2] + [0, 1]
    assert v.value.tolist() == [1] * 3 + [2] * 3 + [1, 1, 1, 1, 2, 1, 2] + [3] * 3 + [3, 1]
    assert J.dirty_reads_from_edn(DIRTY, n=5).n == 5


def test_check_dirty_reads_edn_report():
    s = Stub()
    rep = J.check_dirty_reads_edn(s, DIRTY)
    assert s.calls == [("resolve", False)]  # the resolve only: no graph
    assert rep["valid"] is False
    assert rep["dirty_reads"] == [[1, 2, 1], [2]] and rep["dirty_read_txns"] == [3, 4]
    assert rep["inconsistent_reads"] == [[1, 2, 1], [3, 1]]
    assert rep["short_reads"] == 2 and rep["resolve"]["g1a_reads"] == 2


def test_generators_inject_what_they_say():
    text, inj = J.txn_history_edn(1, n_txns=400)
    tx = J.vhistory_from_txn_edn(text)
    res = M.resolve(tx.vhistory)
    assert tx.vhistory.ntxn == 400 and tx.failed > 0 and tx.info > 0 and tx.unpaired > 0
    assert inj["g1a"] > 0 and inj["g1b"] > 0
    assert res["g1a_reads"] >= inj["g1a"] and res["g1b_reads"] >= inj["g1b"] and res["dangling_reads"] == 0
    text, dirty = J.dirty_reads_edn(2)
    d = J.dirty_reads_from_edn(text)
    rep = J.dirty_reads_report(d, M.resolve(d.ops.vhistory))
    assert d.short_reads > 0 and len(dirty) > 0 and rep["dirty_reads"] == dirty
