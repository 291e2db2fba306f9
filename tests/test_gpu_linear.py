"""hsc_linear_check on the GPU (include/hip_serial.h): every
field of the report must equal the CPU model of linear_model.py -- verdict,
cause, fail_op, prev_ok, peak, final, possible values, expanded, dropped open
reads -- on the shapes where the kernel can go wrong: the table sizes and the
two caps, slot reuse, the pass-through step, keys beyond one round of
workgroups, and calls of different sizes on one context."""
import os

import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import linear_model as LM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J
from test_linear_model import GEN_CASES, GOLDEN, gen_case

pytestmark = pytest.mark.gpu


def run(v, ops, init=None):
    res = v.linear_check(ops, init)
    LM.assert_same(res, LM.check(ops, init))
    assert res["nkeys"] == ops["nkeys"] and res["ms"] >= 0
    return res


def random_keys(seed, nkeys):
    """nkeys random small histories (linear_model.random_ops) and their inits."""
    rng = np.random.default_rng(seed)
    parts, init = [], []
    for _ in range(nkeys):
        ops, i0 = LM.random_ops(rng)
        f, a, b, inv, comp = (list(c) for c in zip(*ops))
        parts.append(dict(f=f, a=a, b=b, invoke=inv, complete=comp))
        init.append(i0)
    return LM.columns(parts), np.array(init, np.int64)


@pytest.mark.parametrize("name", sorted(LM.KNOWN))
def test_known_answers(validator, name):
    text, valid, fail, possible = LM.KNOWN[name]
    ops = J.lin_ops_from_register_edn(text)
    res = run(validator, ops.arrays())
    assert bool(res["verdict"][0] == LM.OK) is valid
    if not valid:
        assert res["fail_op"][0] == fail and res["possible_values"][0] == possible


def test_filetest_history(validator):
    rep = J.check_linear_edn(validator, open(GOLDEN).read())
    assert rep["valid"] is True and rep["bad"] == 0 and rep["events"] == 4


def test_empty_histories(validator):
    for nkeys in (0, 3):
        res = run(validator, LM.columns([None] * nkeys))
        assert res["bad"] == res["unknown"] == res["events"] == 0
        assert res["verdict"].tolist() == [LM.OK] * nkeys and res["final_configs"].tolist() == [1] * nkeys


def test_key_without_ops_among_keys_with_ops(validator):
    res = run(validator, LM.columns([LM.concurrent_writes(3), None, LM.concurrent_writes(2, read=9), None]))
    assert res["verdict"].tolist() == [LM.OK, LM.OK, LM.BAD, LM.OK]
    # (the set before the read holds the empty register alone: both writes are still pending)
    assert res["possible_values"][2] == [None] and res["fail_op"][2] == 6


@pytest.mark.parametrize("nkeys", [1, 2, 300])
def test_keys_in_one_call(validator, nkeys):
    ops, init = random_keys(100 + nkeys, nkeys)
    res = run(validator, ops, init)
    if nkeys == 300:  # more keys than one round of workgroups, both verdicts among them
        assert 0 < res["bad"] < nkeys and res["unknown"] == 0


@pytest.mark.parametrize("procs,stale,seed", GEN_CASES)
def test_generated_histories(validator, procs, stale, seed):
    text, inj = gen_case(procs, stale, seed)
    ops = J.lin_ops_from_register_edn(text)
    res = run(validator, ops.arrays())
    assert res["unknown"] == 0
    if not stale:
        assert res["bad"] == 0


def test_long_program(validator):
    # one key's events pass the 256 the workgroup stages at a time, several times, and end inside a chunk
    text, _ = J.cas_register_history_edn(5, n_ops=700, n_procs=4, info=0.01, max_open=3)
    ops = J.lin_ops_from_register_edn(text)
    res = run(validator, ops.arrays())
    assert res["events"] > 3 * 256 and res["events"] % 256 and res["bad"] == res["unknown"] == 0
    # a bad read behind the first chunk: the failing event is found by its place in the whole program
    bad = ops.arrays()
    reads = np.flatnonzero((bad["f"] == LM.READ) & (bad["complete"] != LM.RT_OPEN))
    bad["a"] = bad["a"].copy()
    bad["a"][reads[len(reads) // 2]] = 77
    res = run(validator, bad)
    assert res["bad"] == 1 and res["fail_op"][0] == reads[len(reads) // 2]


def test_concurrent_writes_at_the_config_cap(validator):
    # k 2^(k-1) + 1 configurations: 1025 and 2305 fit, 5121 does not
    res = run(validator, LM.columns([LM.concurrent_writes(k) for k in (8, 10, 9)]))
    assert res["verdict"].tolist() == [LM.OK, LM.UNKNOWN, LM.OK]
    assert res["cause"].tolist() == [0, LM.CAUSE_CONFIGS, 0]
    assert res["peak_configs"].tolist() == [1025, 1, 2305]


def test_equal_values_collapse(validator):
    # states {nil, 7}: 2^k configurations, kept so by the dedupe; 2^12 is exactly the cap
    res = run(validator, LM.columns([LM.concurrent_writes(k, values=[7] * k) for k in (8, 10, 12, 13)]))
    assert res["verdict"].tolist() == [LM.OK, LM.OK, LM.OK, LM.UNKNOWN]
    assert res["peak_configs"].tolist() == [256, 1024, 4096, 1]


def test_sets_across_every_table_size(validator):
    # work tables of 256 .. 8192 slots hold up to 128 .. 4096 entries: steps on both sides of each
    # limit (distinct values: 2 .. 2305; equal values: 2^k), bad reads among them
    parts = [LM.concurrent_writes(k) for k in range(1, 10)]
    parts += [LM.concurrent_writes(k, values=[3] * k) for k in range(1, 13)]
    parts += [LM.concurrent_writes(k, read=99) for k in (1, 5, 8)]
    res = run(validator, LM.columns(parts))
    assert res["unknown"] == 0 and res["bad"] == 3
    assert sorted(set(res["peak_configs"].tolist()) & {128, 256, 512, 1024, 2048, 4096}) == [
        128, 256, 512, 1024, 2048, 4096]


def test_slots(validator):
    # 32 ops pending at once are judged (the closed write and read share slot 31); a 33rd is not
    res = run(validator, LM.columns([LM.open_cas(31), LM.open_cas(32), LM.open_cas(5)]))
    assert res["verdict"].tolist() == [LM.OK, LM.UNKNOWN, LM.OK]
    assert res["cause"].tolist() == [0, LM.CAUSE_SLOTS, 0]


def test_return_whose_every_configuration_holds_the_op(validator):
    # the read of 1 forces the pending write: its own return finds its bit in every configuration
    res = run(validator, LM.columns([LM.concurrent_writes(1), LM.concurrent_writes(4, values=[5] * 4)]))
    assert res["verdict"].tolist() == [LM.OK, LM.OK] and res["final_configs"].tolist() == [1, 1]


def test_open_reads_are_dropped(validator):
    p = LM.concurrent_writes(2)
    p["f"] += [LM.READ, LM.READ]
    p["a"] += [1, LM.NIL]
    p["b"] += [LM.NIL, LM.NIL]
    p["invoke"] += [0, 1]
    p["complete"] += [LM.RT_OPEN, LM.RT_OPEN]
    res = run(validator, LM.columns([p, dict(f=[LM.READ], a=[4], b=[LM.NIL], invoke=[0], complete=[LM.RT_OPEN])]))
    assert res["dropped_open_reads"] == 3 and res["events"] == 6


def test_two_calls_of_different_sizes(validator):
    big, big_init = random_keys(7, 40)
    small, small_init = random_keys(8, 3)
    first = run(validator, big, big_init)
    run(validator, small, small_init)
    again = run(validator, big, big_init)
    assert first["possible_values"] == again["possible_values"]


def test_reports(validator):
    text, valid, fail, possible = LM.KNOWN["stale_read_acked_overwrite"]
    rep = J.check_linear_edn(validator, text)
    (key,) = rep["keys"].values()
    assert rep["valid"] is False and key["verdict"] is False
    assert key["op"] == {":type": ":ok", ":f": ":read", ":value": 1, ":process": 0, ":time": 6}
    assert key["previous_ok"][":f"] == ":write" and key["previous_ok"][":value"] == 2
    assert key["possible_values"] == [2] and rep["bad"] == 1 and rep["ms"] >= 0
    # the same history from a register that starts at 1 is still invalid; one key of two unknown
    assert J.check_linear_edn(validator, text, init=1)["valid"] is False
    text2, _ = J.cas_register_history_edn(3, n_ops=60, n_procs=3, n_keys=2, independent=True)
    rep2 = J.check_linear_edn(validator, text2, independent=True)
    assert rep2["valid"] is True and sorted(rep2["keys"]) == [0, 1]
    ops = LM.columns([LM.concurrent_writes(10), LM.concurrent_writes(2)])
    lin = J.LinOps(2, *(ops[k] for k in ("key", "f", "a", "b", "invoke", "complete")), ["x", "y"], [{}] * 14)
    rep3 = J.linear_report(lin, validator.linear_check(ops))
    assert rep3["valid"] == "unknown" and rep3["keys"]["x"]["cause"] == "configs" and rep3["keys"]["y"]["verdict"] is True


def test_false_alarm_is_judged_differently(validator):
    """Value matching resolves the read to the overwritten first write of 1 and
    the real-time build reports a cycle no linearization has; the search
    accepts the history, as the literal statement does
    (test_linear_model.py::test_known_answers[false_alarm])."""
    graph = J.check_edn(validator, LM.FALSE_ALARM, realtime=True)
    assert graph["valid"] is True and graph["strict_valid"] is False and graph["realtime_cycles"]
    assert J.check_linear_edn(validator, LM.FALSE_ALARM)["valid"] is True


def test_validation(validator):
    good = LM.columns([LM.concurrent_writes(2)])

    def bad(**change):
        ops = dict(good, **{k: np.array(v, good[k].dtype) if k != "nkeys" else v for k, v in change.items()})
        with pytest.raises(hsc.HscError, match=r"hsc_linear_check -> -1:"):
            validator.linear_check(ops)

    bad(key=[0, 1, 0])                                   # a key >= nkeys
    bad(f=[1, 3, 0])                                     # an unknown f
    bad(invoke=[0, 1, 3], complete=[4, 5, 3])            # invoke == complete on a closed op
    bad(invoke=[0, 1, 4], complete=[4, 5, 3])            # invoke > complete
    bad(nkeys=0)
    lib, ctx = validator.lib, validator.ctx
    rep, ops = hsc.LinReport(), hsc._LinOps(nops=1, nkeys=1)   # NULL arrays
    import ctypes as C
    assert lib.hsc_linear_check(ctx, C.byref(ops), C.byref(rep)) == -1
    assert lib.hsc_linear_check(ctx, None, C.byref(rep)) == -1
    assert lib.hsc_linear_check(ctx, C.byref(ops), None) == -1
    run(validator, good)  # the context still answers
