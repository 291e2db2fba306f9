"""hsc_linear_check_wide on the GPU (include/hip_serial.h, DESIGN.md §5j, the
wide tier): every field of the report must equal the CPU model of
linear_wide_model.py -- the fields of hsc_linear_check's report from the tier
that judged each key, the tier, the escalated and resolved keys, the launch
rounds, the wide expansions -- on the shapes where the tier can go wrong: both
sides of each cap, every table size, keys beyond one round, arenas of
different sizes on one context, and the limits' validation."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import linear_model as LM
import linear_wide_model as WM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J

pytestmark = pytest.mark.gpu

KEY_FIELDS = ("verdict", "cause", "fail_op", "prev_ok", "peak_configs", "final_configs", "possible_values")


def run(v, ops, init=None, **limits):
    res = v.linear_check_wide(ops, init, **limits)
    WM.assert_same(res, WM.check(ops, init, **limits))
    assert res["nkeys"] == ops["nkeys"] and res["ms"] >= res["wide_ms"] >= 0
    return res


def equal_writes(k, **kw):
    return LM.concurrent_writes(k, values=[7] * k, **kw)


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


def test_escalation(validator):
    ops = LM.columns([LM.concurrent_writes(3), LM.concurrent_writes(10), None, LM.concurrent_writes(2, read=9)])
    res = run(validator, ops)
    assert res["tier"].tolist() == [0, 1, 0, 0] and res["escalated"] == res["resolved"] == 1
    assert res["verdict"][1] == LM.OK and res["peak_configs"][1] == 5121
    lds = validator.linear_check(ops)
    assert lds["verdict"][1] == LM.UNKNOWN
    for k in (0, 3):
        for f in KEY_FIELDS:
            assert res[f][k] == lds[f][k], (k, f)


def test_the_wide_cap_is_exact(validator):
    ops = LM.columns([equal_writes(13), equal_writes(14), LM.concurrent_writes(11)])
    res = run(validator, ops, max_configs=8192)
    assert res["verdict"].tolist() == [LM.OK, LM.UNKNOWN, LM.UNKNOWN]
    assert res["cause"].tolist() == [0, LM.CAUSE_CONFIGS, LM.CAUSE_CONFIGS]
    assert res["peak_configs"][0] == 8192 and res["tier"].tolist() == [1, 1, 1]
    res = run(validator, LM.columns([LM.concurrent_writes(11)]), max_configs=16384)
    assert res["verdict"].tolist() == [LM.OK] and res["peak_configs"].tolist() == [11265]


def test_every_wide_table_size(validator):
    # work tables of 256 .. 16384 slots (128 .. 8192 entries), bad reads among them
    ks = list(range(5, 14))
    parts = [equal_writes(k) for k in ks] + [LM.concurrent_writes(k, read=99) for k in (5, 12)]
    res = run(validator, LM.columns(parts), max_configs=1 << 16, wide_only=True)
    assert res["peak_configs"].tolist()[:len(ks)] == [2 ** k for k in ks]
    assert res["bad"] == 2 and res["unknown"] == 0 and res["tier"].all()


@pytest.mark.parametrize("k", [14, 15, 16])
def test_wide_table_sizes_past_the_lds_tier(validator, k):
    res = run(validator, LM.columns([equal_writes(k)]), max_configs=1 << 16, wide_only=True)
    assert res["verdict"].tolist() == [LM.OK] and res["peak_configs"].tolist() == [2 ** k]


def test_slots(validator):
    res = run(validator, LM.columns([LM.open_cas(32), LM.open_cas(47), LM.open_cas(48), LM.open_cas(5)]))
    assert res["verdict"].tolist() == [LM.OK, LM.OK, LM.UNKNOWN, LM.OK]
    assert res["cause"].tolist() == [0, 0, LM.CAUSE_SLOTS, 0]
    assert res["tier"].tolist() == [1, 1, 1, 0] and (res["escalated"], res["resolved"]) == (3, 2)


def test_states(validator):
    def writes(n):
        return dict(f=[LM.WRITE] * n, a=list(range(1, n + 1)), b=[LM.NIL] * n, invoke=[2 * j for j in range(n)],
                    complete=[2 * j + 1 for j in range(n)])

    res = run(validator, LM.columns([writes(hsc.LIN_WIDE_STATES), writes(hsc.LIN_WIDE_STATES + 1)]), wide_only=True)
    assert res["verdict"].tolist() == [LM.OK, LM.UNKNOWN] and res["cause"].tolist() == [0, hsc.LIN_CAUSE_STATES]


def test_budget(validator):
    ops = LM.columns([LM.concurrent_writes(10)])
    total = WM.check(ops)["expanded"]
    res = run(validator, ops, max_expanded=total - 1)
    assert res["verdict"].tolist() == [LM.UNKNOWN] and res["cause"].tolist() == [hsc.LIN_CAUSE_BUDGET]
    assert (res["escalated"], res["resolved"]) == (1, 0)
    res = run(validator, ops, max_expanded=total)
    assert res["verdict"].tolist() == [LM.OK] and res["expanded"] == total


def test_wide_only_parity_on_small_histories(validator):
    ops, init = random_keys(400, 300)
    res = run(validator, ops, init, wide_only=True)
    assert 0 < res["bad"] < 300 and res["unknown"] == 0
    lds = validator.linear_check(ops, init)
    LM.assert_same(res, lds)  # the two tiers agree on every field both report
    for name in sorted(LM.KNOWN):
        text, valid, fail, possible = LM.KNOWN[name]
        res = run(validator, J.lin_ops_from_register_edn(text).arrays(), wide_only=True)
        assert bool(res["verdict"][0] == LM.OK) is valid
        if not valid:
            assert res["fail_op"][0] == fail and res["possible_values"][0] == possible
    for nkeys in (0, 3):
        for wide_only in (False, True):
            res = run(validator, LM.columns([None] * nkeys), wide_only=wide_only)
            assert res["bad"] == res["unknown"] == res["events"] == res["escalated"] == res["rounds"] == 0
            assert res["verdict"].tolist() == [LM.OK] * nkeys and res["tier"].tolist() == [0] * nkeys


def test_rounds(validator):
    ops = LM.columns([LM.concurrent_writes(10), LM.concurrent_writes(9, read=99), equal_writes(13), LM.open_cas(40),
                      LM.concurrent_writes(10, read=99)])
    one = run(validator, ops, max_configs=8192, wide_only=True)
    res = run(validator, ops, max_configs=8192, wide_only=True, arena_bytes=2 * 32 * 8192)
    assert (one["rounds"], res["rounds"]) == (1, 3) and res["escalated"] == 5
    assert res["verdict"].tolist() == [LM.OK, LM.BAD, LM.OK, LM.OK, LM.BAD]
    LM.assert_same(res, one)


def test_arena_regrowth(validator):
    ops = LM.columns([LM.concurrent_writes(10), equal_writes(14), LM.concurrent_writes(10, read=99)])
    first = run(validator, ops, max_configs=1 << 16)
    small = run(validator, ops, max_configs=8192)
    again = run(validator, ops, max_configs=1 << 16)
    assert first["verdict"].tolist() == [LM.OK, LM.OK, LM.BAD] and small["verdict"][1] == LM.UNKNOWN
    WM.assert_same(again, first)


def test_the_references_shape(validator):
    wide = {"max_configs": WM.REFERENCE_CAP}
    text = WM.reference_shape("valid")
    assert J.check_linear_edn(validator, text)["valid"] == "unknown"
    rep = J.check_linear_edn(validator, text, wide=wide)
    (key,) = rep["keys"].values()
    assert rep["valid"] is True and key["tier"] == 1 and key["peak_configs"] == 10312
    assert (rep["escalated"], rep["resolved"]) == (1, 1) and rep["expanded"] == 323441 and rep["wide_ms"] >= 0
    text = WM.reference_shape("stale")
    plain = J.check_linear_edn(validator, text)
    assert plain["valid"] == "unknown" and "escalated" not in plain and "tier" not in next(iter(plain["keys"].values()))
    rep = J.check_linear_edn(validator, text, wide=wide)
    ops = rep["history"]
    ref = WM.check(ops.arrays(), max_configs=WM.REFERENCE_CAP)
    (key,) = rep["keys"].values()
    assert rep["valid"] is False and key["tier"] == 1 and key["cause"] is None
    assert ref["fail_op"].tolist() == [89] and key["op"] is ops.completions[89]
    assert key["possible_values"] == ref["possible_values"][0] and key["peak_configs"] == 9088


def test_validation(validator):
    good = LM.columns([LM.concurrent_writes(10)])

    def bad(**limits):
        with pytest.raises(hsc.HscError, match=r"hsc_linear_check_wide -> -1:"):
            validator.linear_check_wide(good, **limits)

    bad(max_configs=4096)
    bad(max_configs=12288)
    bad(max_configs=1 << 23)
    bad(max_configs=8192, arena_bytes=32 * 8192 - 1)
    lib, ctx = validator.lib, validator.ctx
    s, keep = validator._lin_ops(good, None)
    rep = hsc.LinWideReport()
    lim = hsc._LinWideLimits(flags=2)
    assert lib.hsc_linear_check_wide(ctx, C.byref(s), C.byref(lim), C.byref(rep)) == -1   # an unknown flag
    assert lib.hsc_linear_check_wide(ctx, None, None, C.byref(rep)) == -1
    assert lib.hsc_linear_check_wide(ctx, C.byref(s), None, None) == -1
    null = hsc._LinOps(nops=1, nkeys=1)
    assert lib.hsc_linear_check_wide(ctx, C.byref(null), None, C.byref(rep)) == -1      # NULL arrays
    assert lib.hsc_linear_check_wide(ctx, C.byref(s), None, C.byref(rep)) == 0          # NULL limits: the defaults
    assert rep.escalated == 1 and rep.resolved == 1 and rep.table_bytes == 32 << 20
    run(validator, good)  # the context still answers
    lds = validator.linear_check(good)
    assert lds["verdict"].tolist() == [LM.UNKNOWN] and lds["cause"].tolist() == [LM.CAUSE_CONFIGS]
    LM.assert_same(lds, LM.check(good))
