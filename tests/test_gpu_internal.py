"""hsc_dep_graph_internal / _internal_lists on the GPU (include/hip_serial.h,
DESIGN.md §5i): every field must equal the CPU reference of internal_model.py
exactly, with and without the per-op arrays; the entries must leave what the
resolves keep for their builds alone and answer the same whenever they are
called; and the reports of check_txn_edn / check_append_edn must show the
anomaly only when asked."""
import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import internal_model as IM
import lists_model as LM
import resolve_model as RM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J

pytestmark = pytest.mark.gpu

OK, ABORTED, UNKNOWN = IM.OK, IM.ABORTED, IM.UNKNOWN
SCAN_TILE = 2048  # scan_exclusive_u32: 256 threads x 8 items per workgroup
CHUNK = 1024      # kIcChunk (hsc_intcons.hip): the elements one wave compares
FRESH = 10 ** 15  # elements / values nobody wrote
SCALARS = IM.COUNTS + ("sort_packed",)


def same(a: dict, b: dict):
    """Two result dicts of one entry are equal but for ms."""
    assert set(a) == set(b)
    for k in a:
        if k == "ms":
            continue
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        elif isinstance(a[k], np.ndarray):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
        else:
            assert a[k] == b[k], k


def run_values(v, h, ref=None, in_c=None):
    ref = IM.check_values(h, in_c) if ref is None else ref
    v.dep_graph_resolve(h, arrays=False)
    res = v.graph_internal(arrays=True)
    IM.assert_equal(res, ref, arrays=True)
    bare = v.graph_internal(arrays=False)
    IM.assert_equal(bare, ref, arrays=False)
    assert [res[k] for k in SCALARS] == [bare[k] for k in SCALARS]
    assert res["compared_elements"] == 0
    return res


def run_lists(v, h, ref=None):
    ref = IM.check_lists(h) if ref is None else ref
    v.graph_resolve_lists(h, arrays=False)
    res = v.graph_internal_lists(arrays=True)
    IM.assert_equal(res, ref, arrays=True)
    bare = v.graph_internal_lists(arrays=False)
    IM.assert_equal(bare, ref, arrays=False)
    assert [res[k] for k in SCALARS] == [bare[k] for k in SCALARS]
    return res


# ---- hand-built cases ---------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IM.HAND))
def test_hand_built(validator, name):
    kind, h, want = IM.HAND[name]
    res = (run_values if kind == "value" else run_lists)(validator, h)
    IM.check_expected(res, want)


def test_empty_history(validator):
    for res in (run_values(validator, IM.vh([], [])), run_lists(validator, IM.lh([], []))):
        assert all(res[k] == 0 for k in SCALARS) and res["ms"] == 0
        assert len(res["txn_bad"]) == len(res["listed_op"]) == len(res["bad"]) == 0
    res = run_values(validator, IM.vh([], [OK, ABORTED]))
    assert res["txn_bad"].tolist() == [0, 0] and res["checked_reads"] == 0


# ---- value histories: shapes ------------------------------------------------------
def all_ok(h):
    return [True] * h.ntxn


def test_value_one_long_run(validator):
    """One (txn, key) run of 5000 ops: every read against the op before it."""
    ops, last = [], None
    for i in range(5000):
        if i % 3 == 0:
            last = i + 1
            ops.append((0, 9, "w", last))
        else:
            got = FRESH + i if i % 7 == 0 else last
            ops.append((0, 9, "r", got))
            last = got
    h = IM.vh(ops, [OK])
    res = run_values(validator, h, in_c=all_ok(h))
    assert res["checked_reads"] == sum(1 for o in ops if o[2] == "r") and res["bad_reads"] > 400
    assert res["sort_packed"] == 1


def test_value_runs_of_one_op(validator):
    """5000 runs of one op each: nothing is constrained."""
    h = IM.vh([(t % 50, 100 + t, "r" if t % 2 else "w", t + 1) for t in range(5000)], [OK] * 50)
    res = run_values(validator, h, in_c=all_ok(h))
    assert res["checked_reads"] == 0 and not res["bad"].any() and (res["anchor_op"] == IM.NONE).all()


def value_pairs(nops):
    """One txn, keys ascending with the op index, so sorted position = op
    index: a lone read, then (write, read) pairs at ops (2 j + 1, 2 j + 2) --
    one straddles every multiple of SCAN_TILE; its read and every 97th are bad."""
    ops = [(0, 0, "r", None)]
    for i in range(1, nops):
        k = (i + 1) // 2
        if i % 2:
            ops.append((0, k, "w", k))
        else:
            ops.append((0, k, "r", FRESH + k if i % SCAN_TILE == 0 or k % 97 == 0 else k))
    return IM.vh(ops, [OK])


@pytest.mark.parametrize("nops", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_value_scan_tile_boundaries(validator, nops):
    h = value_pairs(nops)
    res = run_values(validator, h, in_c=all_ok(h))
    for edge in range(SCAN_TILE, nops, SCAN_TILE):
        assert res["bad"][edge] == 1 and res["anchor_op"][edge] == edge - 1
        assert edge in res["listed_op"].tolist()
    assert res["checked_reads"] == (nops - 1) // 2 and res["sort_packed"] == 1


def test_value_sort_paths(validator):
    small = IM.random_values(7, n_txn=60, n_keys=20)
    assert run_values(validator, small)["sort_packed"] == 1
    wide = IM.random_values(7, n_txn=300, n_keys=200, full64=True)
    res = run_values(validator, wide)
    assert res["sort_packed"] == 0 and res["bad_reads"] > 0


@pytest.mark.parametrize("nbad", [IM.LIST_CAP + 1, 5000])
def test_value_listed_cap(validator, nbad):
    ops = []
    for t in range(nbad + 10):
        ops += [(t, 3, "w", t + 1), (t, 3, "r", t + 1 if t >= nbad else None)]
    h = IM.vh(ops, [OK] * (nbad + 10))
    res = run_values(validator, h, in_c=all_ok(h))
    assert res["n_listed"] == IM.LIST_CAP and res["bad_reads"] == nbad and res["bad_txns"] == nbad
    assert res["listed_op"].tolist() == [2 * t + 1 for t in range(IM.LIST_CAP)]


@pytest.mark.parametrize("seed", IM.GPU_SEEDS)
def test_value_random(validator, seed):
    h = IM.random_values(seed)
    res = run_values(validator, h)
    assert res["checked_reads"] >= 100 and 0 < res["bad_reads"] < res["checked_reads"]


# ---- list histories: shapes --------------------------------------------------------
def mismatch_history(L):
    """Reads of L elements, each in a txn and on a key of its own, against a
    prefix read plus own appends (rule 1) and against own appends alone (rule
    2), clean and with exactly one element replaced: the first, the last of the
    prefix, the first appended, the last.  Txn 0 appended every prefix.
    Returns (history, the read ops that must be bad)."""
    a = (L + 2) // 3
    lp = L - a
    spots = sorted({0, max(lp - 1, 0), lp, L - 1})
    ops, status, must = [], [OK], []
    nexte = [1]

    def fresh(n):
        out = list(range(nexte[0], nexte[0] + n))
        nexte[0] += n
        return out

    def variant(rule, spot):
        t, k = len(status), len(status)
        status.append(OK)
        prefix, app = fresh(lp), fresh(a)
        ops.extend((0, k, e) for e in prefix)
        if rule == 1:
            ops.append((t, k, list(prefix)))
        ops.extend((t, k, e) for e in app)
        got = prefix + app
        if spot is not None:
            got[spot] = FRESH + len(ops)
            if rule == 1 or spot >= lp:  # rule 2 compares the last a elements only
                must.append(len(ops))
        ops.append((t, k, got))

    for rule in (1, 2):
        for spot in [None] + spots:
            variant(rule, spot)
    return IM.lh(ops, status), must


@pytest.mark.parametrize("L", [1, 63, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 4095, 4096, 4097, 10000])
def test_list_single_mismatch(validator, L):
    h, must = mismatch_history(L)
    res = run_lists(validator, h)
    assert np.nonzero(res["bad"])[0].tolist() == must
    assert res["bad_reads"] == len(must) and res["listed_op"].tolist() == must
    # every length is right, so every variant compares all it has to: L elements
    # under rule 1, the a appended ones under rule 2
    a = (L + 2) // 3
    nvar = res["checked_reads"] // 2
    assert nvar == 1 + len({0, max(L - a - 1, 0), L - a, L - 1})
    assert res["compared_elements"] == nvar * (L + a)


def test_list_wrong_length_compares_nothing(validator):
    """Two reads after a prefix read; breaking the length of one takes exactly
    its share out of compared_elements."""
    def hist(second):
        return IM.lh([(1, 1, 5), (1, 1, 6), (0, 1, [5, 6]), (0, 1, 10), (0, 1, [5, 6, 10]), (0, 1, 11), (0, 1, second)],
                     [OK, OK])
    clean = run_lists(validator, hist([5, 6, 10, 11]))
    assert (clean["compared_elements"], clean["bad_reads"], clean["checked_reads"]) == (7, 0, 2)
    for second in ([5, 6, 10], [5, 6, 10, 11, 12], []):
        res = run_lists(validator, hist(second))
        assert (res["compared_elements"], res["bad_reads"], res["checked_reads"]) == (3, 1, 2)
        assert res["listed_op"].tolist() == [6] and res["listed_anchor"].tolist() == [4]
    # a wrong element at the right length is compared
    res = run_lists(validator, hist([5, 6, 10, 12]))
    assert (res["compared_elements"], res["bad_reads"]) == (7, 1)


def list_pairs(nops):
    """value_pairs for lists: a lone read, then (append, read) pairs whose read
    must end in the appended element; sorted position = op index."""
    ops = [(0, 0, [])]
    for i in range(1, nops):
        k = (i + 1) // 2
        if i % 2:
            ops.append((0, k, k))
        else:
            ops.append((0, k, [FRESH + k] if i % SCAN_TILE == 0 or k % 97 == 0 else [k]))
    return IM.lh(ops, [OK])


@pytest.mark.parametrize("nops", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1])
def test_list_scan_tile_boundaries(validator, nops):
    res = run_lists(validator, list_pairs(nops))
    for edge in range(SCAN_TILE, nops, SCAN_TILE):
        assert res["bad"][edge] == 1 and res["anchor_op"][edge] == edge - 1
    assert res["checked_reads"] == res["compared_elements"] == (nops - 1) // 2 and res["sort_packed"] == 1


def test_list_sort_paths(validator):
    assert run_lists(validator, IM.random_lists(7, n_txn=60, n_keys=8))["sort_packed"] == 1
    res = run_lists(validator, IM.random_lists(7, n_txn=300, n_keys=12, full64=True))
    assert res["sort_packed"] == 0 and res["bad_reads"] > 0


@pytest.mark.parametrize("seed", IM.GPU_SEEDS)
def test_list_random(validator, seed):
    h = IM.random_lists(seed)
    res = run_lists(validator, h)
    assert res["checked_reads"] >= 100 and 0 < res["bad_reads"] < res["checked_reads"]
    assert res["compared_elements"] > 0


# ---- state ------------------------------------------------------------------------
ESTATE_V = r"hsc_dep_graph_internal -> -5:"
ESTATE_L = r"hsc_dep_graph_internal_lists -> -5:"


def test_state_before_and_after_a_failed_resolve():
    v = hsc.Validator(0)
    try:
        for arrays in (False, True):
            with pytest.raises(hsc.HscError, match=ESTATE_V):
                v.graph_internal(arrays=arrays)
            with pytest.raises(hsc.HscError, match=ESTATE_L):
                v.graph_internal_lists(arrays=arrays)
        kind, good_v, want_v = IM.HAND["v_interleaved"]
        kind, good_l, want_l = IM.HAND["l_append_read_append_read"]
        IM.check_expected(run_values(v, good_v), want_v)
        IM.check_expected(run_lists(v, good_l), want_l)
        for name in sorted(RM.INVALID):
            with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_resolve -> -1:"):
                v.dep_graph_resolve(RM.INVALID[name])
            with pytest.raises(hsc.HscError, match=ESTATE_V):
                v.graph_internal()
            # the other kind's resolve still stands
            IM.assert_equal(v.graph_internal_lists(arrays=True), IM.check_lists(good_l))
        for name in sorted(LM.INVALID):
            with pytest.raises(hsc.HscError, match=r"hsc_dep_graph_resolve_lists -> -1:"):
                v.graph_resolve_lists(LM.INVALID[name])
            with pytest.raises(hsc.HscError, match=ESTATE_L):
                v.graph_internal_lists()
        # and the context goes on working
        IM.check_expected(run_values(v, good_v), want_v)
        IM.check_expected(run_lists(v, good_l), want_l)
    finally:
        v.close()


def _classes(v):
    an, si = v.dep_graph_anomalies(), v.dep_graph_si()
    return ([a.copy() for a in v.dep_graph_edges()],
            [np.asarray(an[k]).copy() for k in ("cls", "comp_label", "comp_class")],
            [np.asarray(si[k]).copy() for k in ("nonadj", "comp_label", "comp_nonadj")])


def _assert_same_graph(a, b):
    for xs, ys in zip(a, b):
        assert len(xs) == len(ys)
        for x, y in zip(xs, ys):
            np.testing.assert_array_equal(x, y)


def _rebuild_with_realtime(v, nc, build):
    inv = np.arange(nc, dtype=np.uint64) * np.uint64(2)
    v.dep_graph_stage_realtime(inv, inv + np.uint64(1))
    build()


@pytest.mark.parametrize("kind", ["value", "lists"])
def test_non_interference_and_repeatability(validator, kind):
    v = validator
    if kind == "value":
        h = RM.generated(11, n_txn=800, n_keys=80)
        ref = IM.check_values(h)
        resolve = lambda: v.dep_graph_resolve(h, arrays=False)  # noqa: E731
        build = lambda: v.dep_graph_build_resolved(full=True)   # noqa: E731
        internal = v.graph_internal
    else:
        h = LM.generated(11, n_txn=800, n_keys=20)
        ref = IM.check_lists(h)
        resolve = lambda: v.graph_resolve_lists(h, arrays=False)  # noqa: E731
        build = lambda: v.graph_build_lists(full=True)            # noqa: E731
        internal = v.graph_internal_lists
    # B: resolve, build
    nc = resolve()["ncommitted"]
    build()
    want = _classes(v)
    assert len(want[0][0]) > 0
    # A: resolve, the internal entry (both forms), build
    resolve()
    first = internal(arrays=True)
    IM.assert_equal(first, ref, arrays=True)
    internal(arrays=False)
    build()
    _assert_same_graph(_classes(v), want)
    # after the build and the analyses, and after a staged real-time order and a rebuild
    same(internal(arrays=True), first)
    _rebuild_with_realtime(v, nc, build)
    assert (v.dep_graph_edges()[2] & 8).any()
    v.dep_graph_anomalies()
    v.dep_graph_si()
    same(internal(arrays=True), first)
    # the entry ran between the resolve and this build too: a plain rebuild still gives B's graph
    build()
    _assert_same_graph(_classes(v), want)


def test_each_entry_answers_for_its_own_history(validator):
    v = validator
    hv, hl = IM.random_values(21, n_txn=300, n_keys=40), IM.random_lists(22, n_txn=300, n_keys=6)
    rv, rl = IM.check_values(hv), IM.check_lists(hl)
    v.dep_graph_resolve(hv, arrays=False)
    v.graph_resolve_lists(hl, arrays=False)
    for _ in range(2):
        IM.assert_equal(v.graph_internal(arrays=True), rv)
        IM.assert_equal(v.graph_internal_lists(arrays=True), rl)
    # a new resolve of one kind moves that entry only
    kind, h2, want = IM.HAND["v_interleaved"]
    v.dep_graph_resolve(h2, arrays=False)
    IM.check_expected(v.graph_internal(arrays=True), want)
    IM.assert_equal(v.graph_internal_lists(arrays=True), rl)


# ---- reports --------------------------------------------------------------------------
TXN_EDN = """
{:type :invoke :f :txn :value [[:w 1 1] [:r 1 nil]] :process 0 :time 1}
{:type :ok     :f :txn :value [[:w 1 1] [:r 1 5]]   :process 0 :time 2}
{:type :invoke :f :txn :value [[:r 1 nil]] :process 1 :time 3}
{:type :ok     :f :txn :value [[:r 1 1]]   :process 1 :time 4}
"""
APPEND_EDN = """
{:type :invoke :f :txn :value [[:append 1 3]] :process 0 :time 1}
{:type :ok     :f :txn :value [[:append 1 3]] :process 0 :time 2}
{:type :invoke :f :txn :value [[:append 1 7] [:r 1 nil]] :process 1 :time 3}
{:type :ok     :f :txn :value [[:append 1 7] [:r 1 [3]]] :process 1 :time 4}
"""
NEW_KEYS = {"internal_anomalies", "internal_anomaly_count", "internal"}
REPORTS = {
    "txn": (J.check_txn_edn, TXN_EDN, {"txn": 0, "key": 1, "op": 1, "anchor_op": 0, "expected": 1, "got": 5}),
    "append": (J.check_append_edn, APPEND_EDN,
               {"txn": 1, "key": 1, "op": 2, "anchor_op": 1, "prefix": None, "appended": [7], "got": [3]}),
}


@pytest.mark.parametrize("name", sorted(REPORTS))
def test_report_shows_the_anomaly_only_when_asked(validator, name):
    check, text, entry = REPORTS[name]
    plain = check(validator, text, isolation=True)
    assert plain["valid"] is True and "internal" not in plain["anomaly_types"]
    assert not NEW_KEYS & set(plain) and "internal_consistent" not in plain["levels"]
    off = check(validator, text, isolation=True, internal=False)
    assert set(off) == set(plain) and off["valid"] is True and off["levels"] == plain["levels"]
    assert off["anomaly_types"] == plain["anomaly_types"]
    on = check(validator, text, isolation=True, internal=True)
    assert set(on) == set(plain) | NEW_KEYS
    assert on["valid"] is False and "internal" in on["anomaly_types"]
    assert on["internal_anomalies"] == [entry] and on["internal_anomaly_count"] == 1
    assert on["internal"]["bad_reads"] == 1 and on["internal"]["checked_reads"] == 1
    assert on["levels"]["serializable"] is False and on["levels"]["snapshot_isolation"] is False
    assert on["levels"]["internal_consistent"] is False
    assert on["levels"]["read_committed"] == plain["levels"]["read_committed"]
    assert on["levels"]["g1c_free"] == plain["levels"]["g1c_free"]
    # the graph part of the report does not move
    assert on["cycles"] == plain["cycles"] and on["resolve"]["ncommitted"] == plain["resolve"]["ncommitted"]
    # without isolation: no levels either way
    bare = check(validator, text, internal=True)
    assert "levels" not in bare and bare["valid"] is False
    # with the real-time order the strict levels are and-ed too
    strict = check(validator, text, isolation=True, realtime=True, internal=True)
    assert strict["levels"]["strict_serializable"] is False
    assert strict["levels"]["strong_snapshot_isolation"] is False
    assert check(validator, text, isolation=True, realtime=True)["levels"]["strict_serializable"] is True
