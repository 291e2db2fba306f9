"""hsc_tally_check and hsc_bank_check on the GPU (include/hip_serial.h,
DESIGN.md §5k): every field of both reports must equal the CPU model of
tally_model.py -- all counts, all listed runs, n_listed, kind, found,
negatives, listed_read -- exactly, on the shapes where a pass can go wrong:
empty inputs, the workgroup and scan-tile boundaries, sub-runs and runs that
span workgroups, the int64 extremes, both sort paths, the list caps, buffer
reuse, other entries' state on the same context, every lane-group size of the
bank kernel and rows longer than a group."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import linear_model as LM
import resolve_model as RM
import tally_model as TM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J
from test_tally_model import BANK_GEN, QUEUE_GEN, SET_GEN

pytestmark = pytest.mark.gpu

MODES = [False, True]  # set, multiset
SCAN_TILE = 2048       # kScanTile of scan_exclusive_u32 (hsc_kernels.hip: 256 threads x 8 items)
I64 = np.int64


def run(v, attempt, ack, seen, multiset):
    a, k, s = (np.asarray(x, I64) for x in (attempt, ack, seen))
    res = v.tally_check(a, k, s, multiset=multiset)
    TM.assert_same_tally(res, TM.tally(a, k, s, multiset))
    assert res["ms"] >= 0 and res["sort_packed"] in (0, 1)
    return res


def run_bank(v, rows, n, total):
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    bal = np.array([x for r in rows for x in r], I64)
    res = v.bank_check(off, bal, n, total)
    TM.assert_same_bank(res, TM.bank(off, bal, n, total))
    assert res["ms"] >= 0
    return res


# ---- tally ------------------------------------------------------------------
@pytest.mark.parametrize("multiset", MODES)
def test_empty_and_single(validator, multiset):
    e = np.zeros(0, I64)
    res = run(validator, e, e, e, multiset)
    assert res["valid"] == 1 and res["distinct"] == 0 and all(res[c]["runs"] == 0 for c in TM.CLASSES)
    full = [np.array([3, 4, 4, 9]), np.array([3, 4, 11]), np.array([4, 4, 4, 7])]
    for i in range(3):  # each one empty in turn
        run(validator, *[e if j == i else full[j] for j in range(3)], multiset)
    for i in range(3):  # a single element, in each source
        res = run(validator, *[np.array([5]) if j == i else e for j in range(3)], multiset)
        assert res["distinct"] == 1
    assert run(validator, [5], [5], [5], multiset)["ok"]["count"] == 1


@pytest.mark.parametrize("multiset", MODES)
@pytest.mark.parametrize("total", [255, 256, 257, SCAN_TILE - 1, SCAN_TILE + 1])
def test_row_totals_at_the_block_and_scan_tile_boundaries(validator, multiset, total):
    rng = np.random.default_rng(total)
    vals = rng.integers(-40, 40, total)
    cut = sorted(rng.integers(0, total + 1, 2))
    run(validator, vals[:cut[0]], vals[cut[0]:cut[1]], vals[cut[1]:], multiset)


def test_one_value_repeated_in_every_source(validator):
    for multiset in MODES:
        res = run(validator, [7] * 3000, [7] * 3000, [7] * 3000, multiset)
        assert res["ok"]["count"] == (3000 if multiset else 1) and res["distinct"] == 1
    # unequal repeat counts: sub-runs of thousands, three values so that every difference shows
    att = [1] * 1000 + [2] * 3000 + [3] * 4000
    ack = [1] * 1000 + [2] * 3000 + [3] * 1000
    seen = [1] * 4000 + [2] * 500 + [3] * 3500
    res = run(validator, att, ack, seen, True)
    assert (res["duplicated"]["count"], res["lost"]["count"], res["recovered"]["count"]) == (3000, 2500, 2500)
    run(validator, att, ack, seen, False)


@pytest.mark.parametrize("multiset", MODES)
@pytest.mark.parametrize("variant", ["whole", "split", "gap"])
def test_a_run_across_workgroups(validator, multiset, variant):
    rng = np.random.default_rng(5)
    base = np.arange(5000, 6000)
    att, ack, seen = base, base, base
    if variant == "split":  # one value in the middle differs: never read, and enqueued twice
        att = np.concatenate([base, [5500]])
        ack = np.concatenate([base, [5500]])
        seen = base[base != 5500]
    elif variant == "gap":
        att = ack = seen = base[base != 5421]
    res = run(validator, rng.permutation(att), rng.permutation(ack), rng.permutation(seen), multiset)
    want = {"whole": [(5000, 5999)], "split": [(5000, 5499), (5501, 5999)], "gap": [(5000, 5420), (5422, 5999)]}
    assert list(zip(res["ok"]["lo"].tolist(), res["ok"]["hi"].tolist())) == want[variant]
    if variant == "split":
        assert res["lost"]["lo"].tolist() == [5500] and res["lost"]["mult"].tolist() == [2 if multiset else 1]


@pytest.mark.parametrize("multiset", MODES)
def test_int64_extremes(validator, multiset):
    lo, hi = TM.INT64_MIN, TM.INT64_MAX
    vals = np.array([hi, 0, lo, -1, hi - 1, 1, lo + 1], I64)
    res = run(validator, vals, vals, vals[::-1], multiset)
    # signed order, and INT64_MAX is not followed by INT64_MIN
    assert list(zip(res["ok"]["lo"].tolist(), res["ok"]["hi"].tolist())) == [(lo, lo + 1), (-1, 1), (hi - 1, hi)]
    res = run(validator, [hi, lo], [], [hi, lo], multiset)
    assert res["recovered"]["runs"] == 2


def test_both_sort_paths(validator):
    rng = np.random.default_rng(9)
    small = rng.integers(0, 500, 3000)
    wide = rng.integers(TM.INT64_MIN, TM.INT64_MAX, 3000, dtype=I64)
    wide[:20] = wide[20:40]  # (some values in more than one source)
    for multiset in MODES:
        took = {run(validator, v[:1200], v[1000:2200], v[1800:], multiset)["sort_packed"] for v in (small, wide)}
        assert took == {0, 1}
        # 64 varying value bits leave no room for the row index: whole rows
        assert run(validator, wide[:1200], wide[1000:2200], wide[1800:], multiset)["sort_packed"] == 0


@pytest.mark.parametrize("multiset", MODES)
def test_more_runs_than_the_list_cap(validator, multiset):
    vals = np.arange(10_000, dtype=I64) * 3 - 15_000  # isolated: every value a run of its own
    rng = np.random.default_rng(3)
    res = run(validator, rng.permutation(vals), rng.permutation(vals), [], multiset)
    lost = res["lost"]
    assert lost["n_listed"] == hsc.TALLY_LIST_CAP and lost["runs"] == lost["count"] == 10_000
    assert np.array_equal(lost["lo"], vals[:hsc.TALLY_LIST_CAP]) and np.array_equal(lost["hi"], lost["lo"])
    assert res["valid"] == 0


def test_buffer_reuse_large_small_large(validator):
    rng = np.random.default_rng(21)
    for n, span, multiset in ((120_000, 30_000, False), (10, 8, True), (150_000, 1 << 40, True), (7, 3, False)):
        vals = rng.integers(0, span, n)
        run(validator, vals[: n // 2], vals[n // 4: n // 2], vals[n // 3:], multiset)


def test_tally_between_a_resolve_and_its_build(validator):
    v = validator
    h = RM.generated(11, n_txn=800, n_keys=80)
    edges = lambda: [a.copy() for a in v.dep_graph_edges()]  # noqa: E731
    v.dep_graph_resolve(h, arrays=False)
    v.dep_graph_build_resolved(full=True)
    want = edges()
    assert len(want[0]) > 0
    v.dep_graph_resolve(h, arrays=False)
    rng = np.random.default_rng(2)
    vals = rng.integers(0, 900, 20_000)  # more rows than the history has ops
    run(v, vals[:9000], vals[5000:12_000], vals[8000:], True)
    run(v, vals[:9000], vals[5000:12_000], vals[8000:], False)
    run_bank(v, [[1, 2, 3]] * 700, 3, 6)
    v.dep_graph_build_resolved(full=True)
    for x, y in zip(edges(), want):
        np.testing.assert_array_equal(x, y)


def test_interleaved_with_linear_check(validator):
    ops = LM.columns([LM.concurrent_writes(3), LM.concurrent_writes(2, read=9)])
    want = LM.check(ops, None)
    rng = np.random.default_rng(4)
    for i in range(3):
        LM.assert_same(validator.linear_check(ops, None), want)
        vals = rng.integers(0, 50, 700)
        run(validator, vals[:300], vals[200:500], vals[400:], bool(i & 1))
        run_bank(validator, [[5, 5], [5, 4], [10]], 2, 10)
    LM.assert_same(validator.linear_check(ops, None), want)


def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    sizes = rng.integers(0, 1500, 3)
    span = int(rng.integers(8, 600))
    a = rng.integers(0, span, sizes[0])
    k = np.concatenate([rng.choice(a, size=min(len(a), int(sizes[1])), replace=True) if len(a) else a[:0],
                        rng.integers(0, span, 3)])  # acks mostly of attempted values, a few orphans
    s = rng.integers(-5, span, sizes[2])
    return a, k, s


@pytest.mark.parametrize("multiset", MODES)
def test_random(validator, multiset):
    populated = set()
    for seed in range(30):
        a, k, s = random_case(seed)
        want = TM.tally(a, k, s, multiset)
        populated |= {c for c in TM.CLASSES if want[c]["count"]}
        TM.assert_same_tally(validator.tally_check(a, k, s, multiset=multiset), want)
    # the comparison is not vacuous: every class the mode can hold showed up
    assert populated == set(TM.CLASSES) - (set() if multiset else {"duplicated"})


# ---- bank -------------------------------------------------------------------
def bank_rows(rng, n, nreads, start=10):
    """Reads of n accounts of `start` each: most fine, the others one of every
    way to be bad, negatives among both."""
    total, rows = n * start, []
    for i in range(nreads):
        r = np.full(n, start, I64)
        if n >= 2:
            j, k = rng.choice(n, 2, replace=False)
            x = int(rng.integers(0, 3 * start))  # above start: a negative balance in a fine row
            r[j] -= x
            r[k] += x
        what = i % 9
        if what == 1:
            r = r[:0]
        elif what == 2:
            r = r[:-1]
        elif what == 3:
            r = np.concatenate([r, [0]])
        elif what == 4:
            r = rng.integers(-3, 4, 1000)
        elif what == 5:
            r[int(rng.integers(0, n))] -= 1 + int(rng.integers(0, 4 * start))  # wrong total, often negative
        rows.append(r.tolist())
    return rows, total


@pytest.mark.parametrize("n", [1, 5, 8, 64, 65, 200])
def test_bank_group_sizes(validator, n):
    rows, total = bank_rows(np.random.default_rng(n), n, 150)
    res = run_bank(validator, rows, n, total)
    assert res["wrong_n"] > 0 and res["wrong_total"] > 0 and (res["reads_with_negative"] > 0 or n == 1)
    assert set(res["kind"].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("nreads", [1, 63, 64, 65, 5000])
def test_bank_read_counts(validator, nreads):
    rows, total = bank_rows(np.random.default_rng(nreads), 5, nreads)
    run_bank(validator, rows, 5, total)


def test_bank_wraparound_and_negatives(validator):
    big = TM.INT64_MAX
    rows = [[big, big, 2], [big, 1, 0], [-big, -big, -2], [-1, -1, 2], [-1, -1, 1], [-4], [0, 0, 0]]
    res = run_bank(validator, rows, 3, 0)
    # 2^63-1 + 2^63-1 + 2 wraps to 0: right only because of the wraparound; the model wraps too
    assert res["kind"].tolist() == [0, 2, 0, 0, 2, 1, 0] and res["found"][1] == TM.INT64_MIN
    assert res["negatives"].tolist() == [0, 0, 3, 2, 2, 1, 0] and res["reads_with_negative"] == 4
    assert res["valid"] == 0 and res["bad"] == 3  # negatives do not enter the verdict


def test_bank_more_bad_reads_than_the_list_cap(validator):
    rows = [[1, 1] if i % 7 else [1, 2] for i in range(6000)]
    res = run_bank(validator, rows, 2, 3)
    assert res["bad"] > hsc.BANK_LIST_CAP == res["n_listed"]
    assert np.array_equal(res["listed_read"], np.flatnonzero(res["kind"])[:hsc.BANK_LIST_CAP])


def test_bank_zero_reads(validator):
    res = run_bank(validator, [], 5, 50)
    assert res["valid"] == 1 and res["n_reads"] == res["bad"] == 0
    assert run_bank(validator, [[]], 0, 0)["valid"] == 1  # a model of no accounts: the empty read is fine


# ---- end to end -------------------------------------------------------------
def same_report(got: dict, want: dict, inner: str, same_inner):
    assert got.keys() == want.keys()
    for k in want:
        if k == inner:
            same_inner(got[k], want[k])
        else:
            assert got[k] == want[k], k


@pytest.mark.parametrize("kw", SET_GEN)
def test_check_set_edn(validator, kw):
    text, inj = J.set_history_edn(7, n_adds=400, n_procs=5, **kw)
    ops = J.set_ops_from_edn(text)
    rep = J.check_set_edn(validator, text)
    same_report(rep, J.set_report(ops, TM.tally(ops.attempt, ops.ack, ops.seen)), "tally", TM.assert_same_tally)
    assert rep["lost"] == TM.interval_set_str(inj["lost"]) and rep["unexpected"] == TM.interval_set_str(inj["unexpected"])
    assert rep["valid"] is (not kw.get("lose") and not kw.get("phantom"))


@pytest.mark.parametrize("kw", QUEUE_GEN)
def test_check_total_queue_edn(validator, kw):
    text, inj = J.queue_history_edn(11, n_enqueues=600, n_procs=5, **kw)
    ops = J.queue_ops_from_edn(text)
    rep = J.check_total_queue_edn(validator, text)
    same_report(rep, J.total_queue_report(ops, TM.tally(ops.attempt, ops.ack, ops.seen, multiset=True)), "tally",
                TM.assert_same_tally)
    for c in ("lost", "duplicated", "unexpected", "recovered"):
        assert sum(m * (hi - lo + 1) for lo, hi, m in rep[c]) == sum(m for _, m in inj[c]), c
    assert rep["valid"] is (not kw.get("lose") and not kw.get("unexpected"))


@pytest.mark.parametrize("kw", BANK_GEN)
def test_check_bank_edn(validator, kw):
    n, start = 5, 10
    text, inj = J.bank_history_edn(13, n=n, start=start, n_ops=300, n_procs=4, **kw)
    ops = J.bank_ops_from_edn(text)
    rep = J.check_bank_edn(validator, text, n, n * start)
    same_report(rep, J.bank_report(ops, TM.bank(ops.off, ops.balance, n, n * start), n, n * start), "bank",
                TM.assert_same_bank)
    # the listed bad reads are exactly the injected ones, found off by the transfer's amount
    want = sorted([(r, "wrong-total", n * start - a) for r, a in inj["skewed"]] +
                  [(r, "wrong-n", n - 1) for r in inj["short"]])
    got = [(int(r), b["type"], b["found"]) for r, b in zip(rep["bank"]["listed_read"], rep["bad_reads"])]
    assert got == want and rep["valid"] is (not want)
