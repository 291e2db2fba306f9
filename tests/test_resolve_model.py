"""The CPU reference of version resolution (resolve_model.py) against
hand-derived answers, against its naive restatement on random histories, and
its lowering against the history a value history was made from."""
import numpy as np
import pytest

import resolve_model as M
from comdb2_amd.workloads import config4_history, value_history


def check_expected(res, want):
    for k, v in want.items():
        got = res[k]
        if isinstance(v, list):
            assert [int(x) for x in got] == v, (k, got, v)
        else:
            assert int(got) == v, (k, got, v)


@pytest.mark.parametrize("name", sorted(M.HAND))
def test_hand_built(name):
    h, want = M.HAND[name]
    res = M.resolve(h)
    check_expected(res, want)
    M.assert_equal(M.naive(h), res)


@pytest.mark.parametrize("name", sorted(M.INVALID))
def test_invalid(name):
    for f in (M.resolve, M.naive):
        with pytest.raises(M.InvalidHistory):
            f(M.INVALID[name])


def test_empty():
    res = M.resolve(M.vh([], []))
    assert res["kept_ops"] == res["ncommitted"] == res["n_listed"] == 0 and len(res["fate"]) == 0


def test_random_against_naive():
    rng = np.random.default_rng(20240611)
    seen = {k: 0 for k in ("g1a_reads", "g1b_reads", "dangling_reads", "internal_reads", "recovered", "dropped")}
    for i in range(2000):
        h = M.random_history(rng, big=bool(i & 1))
        a, b = M.resolve(h), M.naive(h)
        M.assert_equal(a, b)
        for x, y in zip(("txn", "key", "is_write", "observed"), ("txn", "key", "is_write", "observed")):
            np.testing.assert_array_equal(getattr(a["lowered"], x), getattr(b["lowered"], y))
        for k in seen:
            seen[k] += int(a[k]) > 0
    assert all(v > 20 for v in seen.values()), seen  # every case is exercised


def test_generated_has_every_anomaly():
    res = M.resolve(M.generated(1, n_txn=600))
    for k in ("g1a_reads", "g1b_reads", "dangling_reads", "recovered", "dropped", "aborted"):
        assert res[k] > 0, k


def test_lowering_of_all_ok_history_is_the_history():
    h = config4_history(seed=5, n_txn=300, n_keys=4000)
    v = value_history(h)
    assert v.nops == h.nops  # no txn writes a key twice at this seed
    res = M.resolve(v)
    low = res["lowered"]
    assert low.ntxn == h.ntxn and res["kept_ops"] == h.nops
    assert res["g1a_reads"] == res["g1b_reads"] == res["dangling_reads"] == 0
    np.testing.assert_array_equal(low.txn, h.txn)
    np.testing.assert_array_equal(low.key, h.key)
    np.testing.assert_array_equal(low.is_write, h.is_write)
    own = (h.is_write == 0) & (h.observed == h.txn.astype(np.int64))
    np.testing.assert_array_equal(low.observed, h.observed)
    np.testing.assert_array_equal((res["rflag"] & M.RD_INTERNAL) != 0, own)
