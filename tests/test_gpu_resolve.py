"""hsc_dep_graph_resolve / _build_resolved on the GPU (include/hip_serial.h,
DESIGN.md §5g): every array and count must equal the CPU reference of
resolve_model.py exactly, and the graph built from the lowered ops must equal
the graph built from the reference's lowered history."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import resolve_model as M
from comdb2_amd import hsc
from comdb2_amd import jepsen as J
from comdb2_amd.workloads import ValueHistory, config4_history, value_history
from test_resolve_model import check_expected

pytestmark = pytest.mark.gpu

OK, ABORTED, UNKNOWN = M.OK, M.ABORTED, M.UNKNOWN


def run(validator, h, arrays=True):
    res = validator.dep_graph_resolve(h, arrays=arrays)
    ref = M.resolve(h)
    M.assert_equal(res, ref, arrays=arrays)
    return res, ref


# ---- hand-built cases ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.HAND))
def test_hand_built(validator, name):
    h, want = M.HAND[name]
    res, _ = run(validator, h)
    check_expected(res, want)
    bare, _ = run(validator, h, arrays=False)
    check_expected(bare, {k: v for k, v in want.items() if k not in M.OP_ARRAYS})


def test_recovery_chain_needs_more_than_one_round_trip(validator):
    res, _ = run(validator, M.HAND["chain"][0])
    assert res["recovered"] == 9 and res["sweeps"] >= 9


# ---- errors -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(M.INVALID))
def test_invalid_history(validator, name):
    with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_resolve -> -1:"):
        validator.dep_graph_resolve(M.INVALID[name])
    # a failed resolve leaves nothing to build
    with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_build_resolved -> -5:"):
        validator.dep_graph_build_resolved()
    run(validator, M.HAND["g1b"][0])  # and the context goes on working


def test_host_only_context_and_state():
    v = hsc.Validator(-1)
    try:
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_resolve -> -2:"):
            v.dep_graph_resolve(M.HAND["g1a"][0])
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_build_resolved -> -2:"):
            v.dep_graph_build_resolved()
    finally:
        v.close()


def test_build_resolved_before_any_resolve():
    v = hsc.Validator(0)
    try:
        with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_build_resolved -> -5:"):
            v.dep_graph_build_resolved()
    finally:
        v.close()


def test_empty_history(validator):
    res, _ = run(validator, M.vh([], []))
    assert res["kept_ops"] == 0 and res["ncommitted"] == 0 and res["sweeps"] == 0
    st = validator.dep_graph_build_resolved(full=True)
    assert st["edges"] == 0
    # txns without ops
    res, _ = run(validator, M.vh([], [OK, ABORTED, UNKNOWN]))
    assert res["fate"].tolist() == [0, 1, 2] and res["ncommitted"] == 1


# ---- shapes -------------------------------------------------------------------
def writes_then_reads(nw, nr, anomalous=0, status=None):
    """Txn 0 (aborted) writes key i = value i + 1, nw times; txn 1 reads nr of
    them back (every read a G1a read) -- or, with ``anomalous``, txn 0 is OK
    and writes every key twice, txn 1 reading that many first versions."""
    if anomalous:
        ops = [(0, i, "w", 2 * i + 1 + q) for i in range(nw) for q in range(2)]
        ops += [(1, i, "r", 2 * i + 1 + (i >= anomalous)) for i in range(nr)]
        return M.vh(ops, [OK, OK])
    ops = [(0, i, "w", i + 1) for i in range(nw)] + [(1, i % max(nw, 1), "r", i % max(nw, 1) + 1) for i in range(nr)]
    return M.vh(ops, status or [ABORTED, OK])


@pytest.mark.parametrize("nw", [255, 256, 257])
def test_write_count_boundaries(validator, nw):
    res, _ = run(validator, writes_then_reads(nw, 40))
    assert res["writes"] == nw and res["g1a_reads"] == 40


@pytest.mark.parametrize("nops", [4095, 4096, 4097])
def test_op_count_boundaries(validator, nops):
    res, _ = run(validator, writes_then_reads(nops - 1500, 1500, status=[OK, OK]))
    assert res["nops"] == nops and res["kept_ops"] == nops


@pytest.mark.parametrize("k", [63, 64, 65])
def test_anomalous_read_wave_boundaries(validator, k):
    res, _ = run(validator, writes_then_reads(100, 100, anomalous=k))
    assert res["g1b_reads"] == k and res["n_listed"] == k and res["g1b_txns"] == 1


@pytest.mark.parametrize("k", [4095, 4096, 4097])
def test_listed_cap(validator, k):
    res, ref = run(validator, writes_then_reads(300, k))
    assert res["g1a_reads"] == k and res["n_listed"] == min(k, hsc.RESOLVE_LIST_CAP)
    assert ref["n_listed_exact"] == k and len(res["listed_op"]) == res["n_listed"]


# the lookup table's key directory: buckets over [min key, max key]
def test_directory_over_the_whole_key_range(validator):
    nw = 3001
    keys = [i * ((2 ** 64 - 2) // (nw - 1)) for i in range(nw - 1)] + [2 ** 64 - 2]  # 0 and 2^64 - 2 among them
    ops = [(0, k, "w", i + 1) for i, k in enumerate(keys)]
    ops += [(1, k, "r", i + 1) for i, k in enumerate(keys)]
    ops += [(1, k + 1, "r", i + 1) for i, k in enumerate(keys[:-1]) if i % 7 == 0]  # between two keys: dangling
    ops += [(1, k, "r", i + 2) for i, k in enumerate(keys) if i % 11 == 0]          # the key, another key's value
    res, ref = run(validator, M.vh(ops, [OK, OK]))
    assert ref["dangling_reads"] == len(ops) - 2 * nw and ref["kept_ops"] == 2 * nw


def test_directory_with_one_hot_key(validator):
    nw = 5000
    ops = [(i % 3, 77, "w", i + 1) for i in range(nw)] + [(3, 77, "r", i) for i in range(0, nw + 2)]
    res, ref = run(validator, M.vh(ops, [OK, ABORTED, OK, OK]))
    assert ref["dangling_reads"] == 2 and ref["g1a_reads"] > 0 and ref["g1b_reads"] > 0


_GEN = {}


def gen(seed, **kw):
    key = (seed, tuple(sorted(kw.items())))
    if key not in _GEN:
        h = M.generated(seed, **kw)
        _GEN[key] = (h, M.resolve(h))
    return _GEN[key]


def test_many_blocks(validator):
    h, ref = gen(3, n_txn=14000, n_keys=3000, ops_per_txn=5)
    assert h.nops > 70000
    res = validator.dep_graph_resolve(h)
    M.assert_equal(res, ref)
    assert res["recovered"] > 0 and res["g1a_reads"] > 0 and res["g1b_reads"] > 0


# ---- both sort paths ------------------------------------------------------------
def test_small_keys_and_values_sort_packed(validator):
    h, ref = gen(4, n_txn=3000)
    res = validator.dep_graph_resolve(h)
    M.assert_equal(res, ref)
    assert res["sort_path"] == 3


def test_full_64_bit_keys_and_values_sort_whole_rows(validator):
    h, ref = gen(4, n_txn=3000, full64=True)
    res = validator.dep_graph_resolve(h)
    M.assert_equal(res, ref)
    assert res["sort_path"] & 1 == 0  # the (key, value) rows do not fit one word
    assert ref["g1a_reads"] > 0 and ref["g1b_reads"] > 0 and ref["recovered"] > 0


# ---- generated histories ----------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("arrays", [True, False])
def test_generated(validator, seed, arrays):
    h, ref = gen(seed, n_txn=4000)
    res = validator.dep_graph_resolve(h, arrays=arrays)
    M.assert_equal(res, ref, arrays=arrays)
    for k in ("g1a_reads", "g1b_reads", "dangling_reads", "recovered", "dropped"):
        assert res[k] > 0, k


# ---- lowering parity ----------------------------------------------------------------
def edges_of(validator):
    return [a.copy() for a in validator.dep_graph_edges()]


def assert_same_graph(validator, h_value, h_plain, between=None):
    validator.dep_graph_resolve(h_value, arrays=False)
    if between is not None:
        validator.dep_graph_build(between, full=True)
    st = validator.dep_graph_build_resolved(full=True)
    got = edges_of(validator)
    an, si = validator.dep_graph_anomalies(), validator.dep_graph_si()
    st2 = validator.dep_graph_build(h_plain, full=True)
    want = edges_of(validator)
    an2, si2 = validator.dep_graph_anomalies(), validator.dep_graph_si()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert [st[k] for k in ("edges", "ww", "wr", "rw")] == [st2[k] for k in ("edges", "ww", "wr", "rw")]
    for k in ("cls", "comp_label", "comp_class"):
        np.testing.assert_array_equal(an[k], an2[k])
    assert an["comps"] == an2["comps"] and an["txns"] == an2["txns"]
    for k in ("nonadj", "comp_label", "comp_nonadj"):
        np.testing.assert_array_equal(si[k], si2[k])
    return st


def test_lowering_parity_all_ok(validator):
    h = config4_history(seed=6, n_txn=2000, n_keys=3000)
    v = value_history(h)  # (a txn's repeated write of a key is left out: one version either way)
    st = assert_same_graph(validator, v, h)
    assert st["edges"] > 2000 and st["rw"] > 0


def spliced(seed=6):
    """config 4 in value form with aborted and unknown txns: their writes are
    still observed by later reads (G1a reads, recovered txns)."""
    h = config4_history(seed=seed, n_txn=2000, n_keys=3000)
    rng = np.random.default_rng(seed)
    status = rng.choice([OK, ABORTED, UNKNOWN], size=h.ntxn, p=[0.9, 0.05, 0.05]).astype(np.uint8)
    return value_history(h, status)


def test_lowering_parity_with_aborted_and_unknown(validator):
    v = spliced()
    ref = M.resolve(v)
    assert ref["g1a_reads"] > 0 and ref["recovered"] > 0 and ref["dropped"] > 0
    res = validator.dep_graph_resolve(v)
    M.assert_equal(res, ref)
    assert_same_graph(validator, v, ref["lowered"])


def test_plain_build_between_resolve_and_its_build(validator):
    v = spliced(7)
    other = config4_history(seed=8, n_txn=700, n_keys=500)
    assert_same_graph(validator, v, M.resolve(v)["lowered"], between=other)
    # and the other way: the resolve does not disturb a plain build's edges
    validator.dep_graph_build(other, full=True)
    want = edges_of(validator)
    validator.dep_graph_resolve(v, arrays=False)
    for a, b in zip(edges_of(validator), want):
        np.testing.assert_array_equal(a, b)


# ---- Jepsen ---------------------------------------------------------------------------
class ModelResolve:
    """The validator with the resolve and the lowering replaced by the CPU
    reference: check_txn_edn over it assembles the report from the model's
    arrays, the graph analyses being the GPU's own on the model's lowered
    history."""

    def __init__(self, validator):
        self.v = validator

    def dep_graph_resolve(self, vh, arrays=True):
        self.ref = M.resolve(vh)
        return self.ref

    def dep_graph_build_resolved(self, full=True, no_rw=False):
        return self.v.dep_graph_build(self.ref["lowered"], full=full, no_rw=no_rw)

    def __getattr__(self, name):
        return getattr(self.v, name)


def slim(c):
    """What is specified of a cycle entry: which path witnesses a component is not (include/hip_serial.h)."""
    assert len(c["txns"]) == len(c["edge_types"]) == len(c["ops"]) >= 2
    return {k: c[k] for k in ("type", "label")}


def assert_same_report(validator, text, **kw):
    got = J.check_txn_edn(validator, text, **kw)
    want = J.check_txn_edn(ModelResolve(validator), text, **kw)
    for k in ("valid", "anomaly_types", "aborted_reads", "intermediate_reads", "dangling_reads",
              "aborted_read_count", "intermediate_read_count", "dangling_read_count", "g2_keys"):
        assert got[k] == want[k], k
    for k in ("cycles", "si_cycles", "realtime_cycles"):
        assert [slim(c) for c in got.get(k, ())] == [slim(c) for c in want.get(k, ())], k
    for k in ("levels", "strict_valid", "snapshot_isolation_valid", "realtime_anomaly_types"):
        assert got.get(k) == want.get(k), k
    for k in M.COUNTS:
        assert got["resolve"][k] == want["resolve"][k], k
    for k in ("fate", "cid", "txn_of_cid", "txn_g1"):
        np.testing.assert_array_equal(got["resolve_arrays"][k], want["resolve_arrays"][k])
    np.testing.assert_array_equal(got["analysis"]["cls"], want["analysis"]["cls"])
    return got


@pytest.mark.parametrize("seed", [1, 2])
def test_check_txn_edn_generated(validator, seed):
    text, inj = J.txn_history_edn(seed, n_txns=1500, n_keys=40)
    rep = assert_same_report(validator, text, realtime=True, isolation=True)
    assert rep["aborted_read_count"] >= inj["g1a"] > 0 and rep["intermediate_read_count"] >= inj["g1b"] > 0
    assert rep["valid"] is False and {"G1a", "G1b"} <= set(rep["anomaly_types"])
    assert rep["resolve"]["recovered"] > 0 and rep["resolve"]["dropped"] > 0


def test_check_txn_edn_cycle_free_with_g1a(validator):
    from test_txn_edn import TXNS
    rep = assert_same_report(validator, TXNS, isolation=True)
    assert rep["cycles"] == [] and rep["valid"] is False
    assert rep["levels"]["read_committed"] is False and rep["levels"]["serializable"] is True
    assert [e["reader"] for e in rep["aborted_reads"]] == [1]


WRITE_SKEW_EDN = """
{:type :invoke :f :txn :value [[:r 1 nil] [:r 2 nil] [:w 1 10]] :process 0 :time 1}
{:type :invoke :f :txn :value [[:r 1 nil] [:r 2 nil] [:w 2 20]] :process 1 :time 2}
{:type :ok :f :txn :value [[:r 1 nil] [:r 2 nil] [:w 1 10]] :process 0 :time 3}
{:type :ok :f :txn :value [[:r 1 nil] [:r 2 nil] [:w 2 20]] :process 1 :time 4}
"""


def test_check_txn_edn_write_skew_only(validator):
    rep = assert_same_report(validator, WRITE_SKEW_EDN, isolation=True)
    assert rep["anomaly_types"] == ["G2"] and rep["valid"] is False
    assert rep["levels"] == {"g1c_free": True, "snapshot_isolation": True, "serializable": False,
                             "read_committed": True}
    (c,) = rep["cycles"]
    assert sorted(c["txns"]) == [0, 1] and c["edge_types"] == ["rw", "rw"]


@pytest.mark.parametrize("seed", [2, 3])
def test_check_dirty_reads_edn(validator, seed):
    text, injected = J.dirty_reads_edn(seed)
    rep = J.check_dirty_reads_edn(validator, text)
    assert rep["short_reads"] > 0 and len(injected) > 0
    assert rep["dirty_reads"] == injected and rep["valid"] is False
    ref = M.resolve(rep["history"].ops.vhistory)
    for k in M.COUNTS:
        assert rep["resolve"][k] == ref[k], k
    clean, none = J.dirty_reads_edn(seed, dirty=0.0)
    assert none == [] and J.check_dirty_reads_edn(validator, clean)["valid"] is True
