"""The CPU side of hsc_linear_check: the model of
linear_model.py against the literal statement of linearizability and known
answers, the EDN conversion and the report of comdb2_amd/jepsen.py on model
dicts, the generator's promise that no key of the GPU suite's histories comes
out UNKNOWN, and the host-only context."""
import os

import numpy as np
import pytest

import linear_model as LM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jepsen_filetest_history.txt")


def model_report(text, init=None, independent=False):
    ops = J.lin_ops_from_register_edn(text, independent)
    iv = None if init is None else np.full(ops.nkeys, init, np.int64)
    return ops, J.linear_report(ops, LM.check(ops.arrays(), iv) | {"ms": 0.0})


def test_model_equals_the_literal_statement():
    rng = np.random.default_rng(20260)
    verdicts = {True: 0, False: 0}
    for _ in range(3200):
        ops, init = LM.random_ops(rng)
        ref = LM.check(LM.one_key(ops), None if init == LM.NIL else [init])
        assert ref["unknown"] == 0
        want = LM.literal(ops, init)
        assert (ref["verdict"][0] == LM.OK) == want, (ops, init)
        verdicts[want] += 1
        first = LM.literal_first_failure(ops, init)
        assert (first is None) == want, (ops, init)
        assert ref["fail_op"][0] == (LM.NONE if first is None else first), (ops, init)
    assert min(verdicts.values()) > 500  # both answers are exercised


def test_filetest_history_is_valid():
    _, rep = model_report(open(GOLDEN).read())
    assert rep["valid"] is True and rep["ok"] == 2


@pytest.mark.parametrize("name", sorted(LM.KNOWN))
def test_known_answers(name):
    text, valid, fail, possible = LM.KNOWN[name]
    ops, rep = model_report(text)
    (key,) = rep["keys"].values()
    assert rep["valid"] is valid and key["verdict"] is valid
    # the literal statement decides
    rows = list(zip(ops.f.tolist(), ops.a.tolist(), ops.b.tolist(), ops.invoke.tolist(), ops.complete.tolist()))
    assert LM.literal(rows) is valid
    if valid:
        assert key["op"] is None and key["possible_values"] is None
    else:
        assert key["op"] is ops.completions[fail] and key["op"][":type"] == ":ok"
        assert key["possible_values"] == possible
        assert LM.literal_first_failure(rows) == fail


def test_false_alarm_value_matching_picks_the_wrong_writer():
    """The history the two entries judge differently: value matching sends the
    read of 1 to the first writer of 1 (the latest before it), which the write
    of 2 overwrote before the read began, while the search linearizes the
    second write of 1, still in flight, before the read."""
    j = J.history_from_jepsen_edn(LM.FALSE_ALARM)
    h = j.history
    read = int(np.flatnonzero(h.is_write == 0)[0])
    assert h.ntxn == 4 and h.txn[read] == 2
    assert h.observed[read] == 0  # txn 0 = w(1) over [1, 2]; txn 1 = w(2) completed at 4 < the read's invoke 6
    assert j.complete[1] < j.invoke[2]
    _, rep = model_report(LM.FALSE_ALARM)
    assert rep["valid"] is True


@pytest.mark.parametrize("k", range(1, 11))
def test_counting_identity(k):
    ref = LM.check(LM.columns([LM.concurrent_writes(k)]))
    want = k * 2 ** (k - 1) + 1
    if want <= LM.CAP:
        assert ref["verdict"][0] == LM.OK and ref["peak_configs"][0] == want
    else:
        assert ref["verdict"][0] == LM.UNKNOWN and ref["cause"][0] == LM.CAUSE_CONFIGS
    # without the cap the identity holds for every k
    cap, LM.CAP = LM.CAP, 1 << 30
    try:
        assert LM.check(LM.columns([LM.concurrent_writes(k)]))["peak_configs"][0] == want
    finally:
        LM.CAP = cap


def test_equal_values_collapse():
    ref = LM.check(LM.columns([LM.concurrent_writes(10, values=[7] * 10)]))
    # states {nil, 7}: (nil, {}) and (7, S) for every non-empty S
    assert ref["verdict"][0] == LM.OK and ref["peak_configs"][0] == 2 ** 10


def test_slots():
    ref = LM.check(LM.columns([LM.open_cas(31), LM.open_cas(32)]))
    # 31 open ops + the write: 32 slots, judged; 32 + the write: a 33rd
    assert ref["verdict"].tolist() == [LM.OK, LM.UNKNOWN] and ref["cause"].tolist() == [0, LM.CAUSE_SLOTS]
    # after the write of 1 only the open cas [1 2] may follow: the read's step holds (1, {}) and (2, {cas})
    assert ref["peak_configs"].tolist() == [2, 0] and ref["final_configs"].tolist() == [1, 0]


def test_conversion_forms():
    text = ("{:type :invoke :f :write :value [7 1] :process 0}\n"
            "{:type :invoke :f :cas :value [9 [1 2]] :process 1}\n"
            "{:type :ok :f :write :value [7 1] :process 0}\n"
            "{:type :fail :f :cas :value [9 [1 2]] :process 1}\n"
            "{:type :invoke :f :read :value [7 nil] :process 1}\n"
            "{:type :ok :f :read :value [7 1] :process 1}\n"
            "{:type :invoke :f :cas :value [7 [1 3]] :process 0}\n"
            "{:type :info :f :cas :value [7 [1 3]] :process 0}\n"
            "{:type :invoke :f :read :value [9 nil] :process 2}\n")
    ops = J.lin_ops_from_register_edn(text, independent=True)
    assert ops.keys == [7, 9] and not ops.use_time
    assert (ops.ok, ops.failed, ops.info, ops.unpaired) == (2, 1, 1, 1)
    assert ops.key.tolist() == [0, 0, 0, 1] and ops.f.tolist() == [LM.WRITE, LM.READ, LM.CAS, LM.READ]
    assert ops.a.tolist() == [1, 1, 1, LM.NIL] and ops.b.tolist() == [LM.NIL, LM.NIL, 3, LM.NIL]
    assert ops.invoke.tolist() == [0, 4, 6, 8] and ops.complete.tolist() == [2, 5, LM.RT_OPEN, LM.RT_OPEN]
    ref = LM.check(ops.arrays())
    assert ref["dropped_open_reads"] == 1 and ref["bad"] == 0
    # :key form, :time positions
    keyed = J.lin_ops_from_register_edn("{:type :invoke :f :write :value 1 :key 3 :process 0 :time 10}\n"
                                        "{:type :ok :f :write :value 1 :key 3 :process 0 :time 20}\n")
    assert keyed.keys == [3] and keyed.use_time and keyed.invoke.tolist() == [10] and keyed.complete.tolist() == [20]


GEN_CASES = [(procs, stale, seed) for procs in (2, 5, 9) for stale in (0.0, 0.05) for seed in (1, 2)]


def gen_case(procs, stale, seed):
    """The generated histories tests/test_gpu_linear.py runs: n_procs + open
    non-read ops per key <= 9, five values: a step holds at most 6 * 2^9 = 3072
    configurations."""
    return J.cas_register_history_edn(seed, n_ops=400, n_procs=procs, n_keys=3, n_values=5, info=0.05,
                                      stale=stale, max_open=9 - procs)


@pytest.mark.parametrize("procs,stale,seed", GEN_CASES)
def test_generated_histories_stay_inside_the_caps(procs, stale, seed):
    text, inj = gen_case(procs, stale, seed)
    assert ":uid" not in text
    ops, rep = model_report(text)
    assert rep["unknown"] == 0
    assert max(k["peak_configs"] for k in rep["keys"].values()) <= 6 * 2 ** 9
    if not stale:
        assert rep["valid"] is True and not inj["stale"]
    assert ops.info == inj["info"] <= 3 * max(9 - procs, 0)


def test_generated_stale_reads_are_found():
    bad = 0
    for seed in range(6):
        text, inj = J.cas_register_history_edn(seed, n_ops=300, n_procs=3, n_values=5, info=0.0, stale=0.1)
        _, rep = model_report(text)
        assert inj["stale"]
        bad += rep["valid"] is False
    assert bad >= 5  # (an overlapping write may have put the value back)


def test_host_only_context_has_no_device():
    v = hsc.Validator(-1)
    try:
        with pytest.raises(hsc.HscError, match=r"hsc_linear_check -> -2:"):
            v.linear_check(LM.columns([LM.concurrent_writes(2)]))
    finally:
        v.close()
