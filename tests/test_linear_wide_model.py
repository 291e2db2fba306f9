"""The CPU side of hsc_linear_check_wide (the wide tier): the
parametrised model of linear_wide_model.py against linear_model.py at the LDS
tier's caps and against the literal statement of linearizability at the wide
ones, its two-tier report, and what it says of the generated histories the GPU
suite runs -- so those inputs are known to stay inside the wide caps by the
model alone."""
import numpy as np
import pytest

import linear_model as LM
import linear_wide_model as WM
from comdb2_amd import jepsen as J


def at_lds_caps(ops, init=None):
    return WM.check(ops, init, max_configs=LM.CAP, max_expanded=WM.NO_BUDGET, wide_only=True, slots=LM.SLOTS,
                    max_states=None)


def test_equals_the_lds_model_at_its_caps():
    rng = np.random.default_rng(4801)
    for _ in range(400):
        ops, init = LM.random_ops(rng)
        iv = None if init == LM.NIL else [init]
        LM.assert_same(at_lds_caps(LM.one_key(ops), iv), LM.check(LM.one_key(ops), iv))
    shapes = [LM.concurrent_writes(k) for k in (8, 9, 10)] + [LM.open_cas(31), LM.open_cas(32)]
    ref = LM.check(LM.columns(shapes))
    LM.assert_same(at_lds_caps(LM.columns(shapes)), ref)
    assert ref["verdict"].tolist() == [LM.OK, LM.OK, LM.UNKNOWN, LM.OK, LM.UNKNOWN]
    assert ref["cause"].tolist() == [0, 0, LM.CAUSE_CONFIGS, 0, LM.CAUSE_SLOTS]


def test_equals_the_literal_statement_at_the_wide_caps():
    rng = np.random.default_rng(4802)
    verdicts = {True: 0, False: 0}
    for _ in range(400):
        ops, init = LM.random_ops(rng)
        ref = WM.check(LM.one_key(ops), None if init == LM.NIL else [init], wide_only=True)
        first = LM.literal_first_failure(ops, init)
        assert ref["unknown"] == 0 and ref["tier"].tolist() == [1]
        assert (ref["verdict"][0] == LM.OK) == (first is None), (ops, init)
        assert ref["fail_op"][0] == (LM.NONE if first is None else first), (ops, init)
        verdicts[first is None] += 1
    assert min(verdicts.values()) > 50


def test_two_tiers():
    ops = LM.columns([LM.concurrent_writes(3), LM.concurrent_writes(10), None, LM.concurrent_writes(2, read=9)])
    ref, lds = WM.check(ops), LM.check(ops)
    assert ref["tier"].tolist() == [0, 1, 0, 0] and (ref["escalated"], ref["resolved"], ref["rounds"]) == (1, 1, 1)
    assert ref["verdict"].tolist() == [LM.OK, LM.OK, LM.OK, LM.BAD] and ref["peak_configs"][1] == 10 * 2 ** 9 + 1
    for k in (0, 2, 3):
        for f in ("verdict", "cause", "fail_op", "prev_ok", "peak_configs", "final_configs", "possible_values"):
            assert ref[f][k] == lds[f][k]
    alone = WM.check(LM.columns([LM.concurrent_writes(10)]), wide_only=True)
    assert ref["table_bytes"] == 32 << 20 and ref["wide_expanded"] == alone["expanded"] > 0
    # the wide caps: a 49th pending op, a step past max_configs, the budget, the states
    ref = WM.check(LM.columns([LM.open_cas(32), LM.open_cas(47), LM.open_cas(48), LM.open_cas(5)]))
    assert ref["verdict"].tolist() == [LM.OK, LM.OK, LM.UNKNOWN, LM.OK] and ref["cause"][2] == LM.CAUSE_SLOTS
    assert ref["tier"].tolist() == [1, 1, 1, 0] and (ref["escalated"], ref["resolved"], ref["rounds"]) == (3, 2, 1)
    ops = LM.columns([LM.concurrent_writes(11)])
    assert WM.check(ops, max_configs=8192)["cause"].tolist() == [LM.CAUSE_CONFIGS]
    assert WM.check(ops, max_configs=16384)["peak_configs"].tolist() == [11 * 2 ** 10 + 1]
    ops = LM.columns([LM.concurrent_writes(10)])
    total = WM.check(ops)["expanded"]
    over = WM.check(ops, max_expanded=total - 1)
    assert over["verdict"].tolist() == [LM.UNKNOWN] and over["cause"].tolist() == [WM.CAUSE_BUDGET]
    assert over["escalated"] == 1 and over["resolved"] == 0
    assert WM.check(ops, max_expanded=total)["verdict"].tolist() == [LM.OK]


def sequential_writes(n):
    return dict(f=[LM.WRITE] * n, a=list(range(1, n + 1)), b=[LM.NIL] * n, invoke=[2 * j for j in range(n)],
                complete=[2 * j + 1 for j in range(n)])


def test_state_limit():
    ops = LM.columns([sequential_writes(WM.WIDE_STATES), sequential_writes(WM.WIDE_STATES + 1)])
    ref = WM.check(ops, wide_only=True)
    assert ref["verdict"].tolist() == [LM.OK, LM.UNKNOWN] and ref["cause"].tolist() == [0, WM.CAUSE_STATES]
    assert ref["events"] == 2 * WM.WIDE_STATES and ref["rounds"] == 1 and ref["escalated"] == 2


def test_rounds_follow_the_arena():
    ops = LM.columns([LM.concurrent_writes(10)] * 5)
    ref = WM.check(ops, max_configs=8192, arena_bytes=2 * WM.table_bytes(8192))
    assert ref["rounds"] == 3 and ref["escalated"] == ref["resolved"] == 5


@pytest.fixture(scope="module")
def reference_ops():
    return {name: J.lin_ops_from_register_edn(WM.reference_shape(name)) for name in WM.REFERENCE_SHAPES}


def test_reference_shape_valid(reference_ops):
    ops = reference_ops["valid"].arrays()
    lds = LM.check(ops)
    assert lds["verdict"].tolist() == [LM.UNKNOWN] and lds["cause"].tolist() == [LM.CAUSE_CONFIGS]
    ref = WM.check(ops, max_configs=WM.REFERENCE_CAP)
    assert ref["verdict"].tolist() == [LM.OK] and ref["tier"].tolist() == [1]
    assert ref["peak_configs"].tolist() == [10312] and ref["expanded"] == 323441


def test_reference_shape_stale(reference_ops):
    ops = reference_ops["stale"].arrays()
    assert LM.check(ops)["verdict"].tolist() == [LM.UNKNOWN]
    ref = WM.check(ops, max_configs=WM.REFERENCE_CAP)
    assert ref["verdict"].tolist() == [LM.BAD] and ref["fail_op"].tolist() == [89]
    assert ref["peak_configs"].tolist() == [9088]
