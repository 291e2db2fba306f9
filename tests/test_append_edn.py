"""Elle's list-append EDN form (jepsen.lhistory_from_append_edn) and the
generator jepsen.append_history_edn, on the CPU."""
import numpy as np
import pytest

import lists_model as M
from comdb2_amd import jepsen as J
from test_anomaly import ref_anomalies

# the writers of key 1 complete in the opposite order to the one their appends were applied in
REORDERED = """
{:type :invoke :f :txn :value [[:append 1 1] [:append 2 1]] :process 0 :time 1}
{:type :invoke :f :txn :value [[:r 2 nil] [:append 1 2]] :process 1 :time 2}
{:type :ok :f :txn :value [[:r 2 [1]] [:append 1 2]] :process 1 :time 3}
{:type :ok :f :txn :value [[:append 1 1] [:append 2 1]] :process 0 :time 4}
{:type :invoke :f :txn :value [[:r 1 nil]] :process 2 :time 5}
{:type :ok :f :txn :value [[:r 1 [1 2]]] :process 2 :time 6}
"""

MIXED = """
{:type :invoke :f :txn :value [[:append 5 1] [:r 5 nil]] :process 0 :time 10}
{:type :ok :f :txn :value [[:append 5 1] [:r 5 [1]]] :process 0 :time 20}
{:type :invoke :f :txn :value [[:append 5 2] [:r 6 nil]] :process 1 :time 11}
{:type :fail :f :txn :value [[:append 5 2] [:r 6 nil]] :process 1 :time 21}
{:type :invoke :f :txn :value [[:r 6 nil] [:append 6 3]] :process 2 :time 12}
{:type :info :f :txn :value [[:r 6 nil] [:append 6 3]] :process 2 :time 22}
{:type :invoke :f :txn :value [[:append 6 4]] :process 3 :time 13}
{:type :invoke :f :txn :value [[:r 6 nil] [:r 7 nil]] :process 4 :time 30}
{:type :ok :f :txn :value [[:r 6 [3]] [:r 7 []]] :process 4 :time 31}
{:type :invoke :f :read :value nil :process 5 :time 32}
{:type :ok :f :read :value 3 :process 5 :time 33}
"""


def test_parse_reordered():
    a = J.lhistory_from_append_edn(REORDERED)
    h = a.lhistory
    # ids by completion: the reader of key 2 first
    assert (a.ok, a.failed, a.info, a.unpaired) == (3, 0, 0, 0)
    assert h.txn.tolist() == [0, 0, 1, 1, 2] and h.key.tolist() == [2, 1, 1, 2, 1]
    assert h.is_write.tolist() == [0, 1, 1, 1, 0] and h.value.tolist() == [0, 2, 1, 1, 0]
    assert h.list_off.tolist() == [0, 1, 1, 1, 1, 3] and h.elems.tolist() == [1, 1, 2]
    assert a.invoke.tolist() == [2, 1, 5] and a.complete.tolist() == [3, 4, 6]
    ref = M.resolve(h)
    # version order of key 1 from the read: txn 1 then txn 0, against completion order
    assert M.edge_list(ref) == [(0, 2, M.WR), (1, 0, M.WW | M.WR)]


def test_parse_statuses_and_empty_reads():
    a = J.lhistory_from_append_edn(MIXED)
    h = a.lhistory
    assert (a.ok, a.failed, a.info, a.unpaired) == (2, 1, 1, 1) and h.ntxn == 5  # the :read op is not a txn
    # ids: (time of completion for :ok / :fail, of the invoke for the others)
    assert h.status.tolist() == [J.TXN_UNKNOWN, J.TXN_UNKNOWN, J.TXN_OK, J.TXN_ABORTED, J.TXN_OK]
    # ops that did not complete :ok give their appends and no reads; nil / [] reads are empty
    assert h.txn.tolist() == [0, 1, 2, 2, 3, 4, 4]
    assert h.is_write.tolist() == [1, 1, 1, 0, 1, 0, 0]
    assert h.key.tolist() == [6, 6, 5, 5, 5, 6, 7] and h.value.tolist() == [3, 4, 1, 0, 2, 0, 0]
    assert h.list_off.tolist() == [0, 0, 0, 0, 1, 1, 2, 2] and h.elems.tolist() == [1, 3]
    assert a.complete.tolist()[:2] == [J.RT_OPEN, J.RT_OPEN]
    ref = M.resolve(h)
    assert ref["fate"].tolist() == [3, 2, 0, 1, 0] and ref["rflag"].tolist() == [0, 0, 0, M.I, 0, 0, 0]


def test_parse_errors():
    with pytest.raises(ValueError, match="unknown micro-op"):
        J.lhistory_from_append_edn('{:type :ok :f :txn :value [[:w 1 2]] :process 0 :time 1}')
    with pytest.raises(ValueError, match="without an element"):
        J.lhistory_from_append_edn('{:type :ok :f :txn :value [[:append 1 nil]] :process 0 :time 1}')


@pytest.mark.parametrize("seed", [5, 6])
def test_clean_generated_history_is_serializable(oracle_mod, seed):
    text, inj = J.append_history_edn(seed, n_txns=1500, dirty=0, intermediate=0, dangling=0, duplicate=0,
                                     incompatible=0, cycles=False)
    assert not any(inj.values())
    a = J.lhistory_from_append_edn(text)
    ref = M.resolve(a.lhistory)
    for k in ("g1a_reads", "g1b_reads", "dangling_reads", "duplicate_reads", "incompatible_reads"):
        assert ref[k] == 0, k
    assert ref["recovered"] > 0 and ref["dropped"] > 0 and ref["aborted"] > 0
    s, d, t = ref["edges"]
    assert len(ref_anomalies(oracle_mod, ref["ncommitted"], s, d, t).comp_label) == 0
    # completion order is not version order: ids are completion order here, and ww edges go down in id
    assert ((t & M.WW != 0) & (ref["txn_of_cid"][s] > ref["txn_of_cid"][d])).sum() > 10


def test_each_switch_injects_its_anomaly():
    off = dict(dirty=0, intermediate=0, dangling=0, duplicate=0, incompatible=0, cycles=False)
    for switch, value, counter in (("dirty", 0.5, "g1a_reads"), ("intermediate", 1.0, "g1b_reads"),
                                   ("dangling", 0.01, "dangling_reads"), ("duplicate", 0.01, "duplicate_reads"),
                                   ("incompatible", 0.02, "incompatible_reads")):
        text, inj = J.append_history_edn(7, n_txns=800, **dict(off, **{switch: value}))
        ref = M.resolve(J.lhistory_from_append_edn(text).lhistory)
        assert inj[switch] > 0 and ref[counter] > 0, switch
        others = {"g1a_reads", "g1b_reads", "dangling_reads", "duplicate_reads", "incompatible_reads"} - {counter}
        assert all(ref[k] == 0 for k in others), switch
