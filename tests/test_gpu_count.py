"""hsc_counter_check and hsc_queue_check on the GPU against the models of
tests/count_model.py: every field of both reports, on the smallest shapes where
a pass of hsc_count.hip can go wrong.  Workgroups hold 256 rows, a scan tile
2048 elements (and the scans run over n + 1 of them)."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import count_model as CM
import linear_model as LM
import resolve_model as RM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J
from test_count_model import ModelValidator

pytestmark = pytest.mark.gpu

SCAN_TILE = 2048
SIZES = [255, 256, 257, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1]
I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)


def run_counter(v, cols, nkeys=1, null_key=False):
    t, f, p, val, key = cols
    got = v.counter_check(t, f, p, val, None if null_key else key, nkeys)
    want = CM.counter_np(t, f, p, val, key, nkeys)
    CM.assert_same(got, want, CM.COUNTER_FIELDS, CM.COUNTER_SCALARS)
    return got


def run_queue(v, rows, nkeys=1, null_key=False, finals=(True, False)):
    f, val, key = rows
    out = {}
    for fifo in (False, True):
        for final in finals:
            got = v.queue_check(f, val, None if null_key else key, nkeys, fifo=fifo, final=final)
            want = CM.queue_np(f, val, key, nkeys, fifo=fifo, final=final)
            CM.assert_same(got, want, CM.QUEUE_FIELDS, CM.QUEUE_SCALARS)
            out[fifo, final] = got
    return out


def counter_cols(rows, key=None):
    """(type, f, process, value) tuples -> columns."""
    a = np.array(rows, dtype=object).reshape(-1, 4)
    return (a[:, 0].astype(np.uint8), a[:, 1].astype(np.uint8), a[:, 2].astype(np.uint32),
            np.array([int(x) for x in a[:, 3]], np.int64),
            np.zeros(len(a), np.uint32) if key is None else np.asarray(key, np.uint32))


def queue_rows(rows, key=None):
    a = np.array(rows, dtype=object).reshape(-1, 2)
    return (a[:, 0].astype(np.uint8), np.array([int(x) for x in a[:, 1]], np.int64),
            np.zeros(len(a), np.uint32) if key is None else np.asarray(key, np.uint32))


# ---- both entries: sizes ------------------------------------------------------
def test_empty_and_single_row(validator):
    """n == 0 makes no launch; one row is the sorts' and scans' smallest input."""
    for nkeys in (1, 3):
        got = run_counter(validator, counter_cols([]), nkeys, null_key=nkeys == 1)
        assert got["reads"] == 0 and not got["verdict"].any() and (got["malformed_op"] == hsc.NO_ROW).all()
        run_queue(validator, queue_rows([]), nkeys, null_key=nkeys == 1)
    for row in ((CM.INVOKE, CM.ADD, 0, 5), (CM.OK, CM.READ, 0, 5), (CM.INFO, CM.OTHER, 0, CM.NIL)):
        run_counter(validator, counter_cols([row]))
    for row in ((CM.ENQ, 7), (CM.DEQ, 7)):
        run_queue(validator, queue_rows([row]))


@pytest.mark.parametrize("n", SIZES)
def test_row_counts_at_the_workgroup_and_scan_tile_edges(validator, n):
    """n rows with 1 and with 3 interleaved keys: the last workgroup and the
    last scan tile full, one short, one over; 2 * 2048 + 1: two scan levels."""
    for nkeys in (1, 3):
        cols = CM.gen_counter(n, (n + 1) // 2, nprocs=5, nkeys=nkeys)
        cols = tuple(c[:n] for c in cols)
        got = run_counter(validator, CM.set_reads(cols, nkeys), nkeys)
        assert got["reads"] > 0 and 0 < got["bad_reads"] < got["reads"] and got["unknown"] == 0
        run_queue(validator, CM.gen_queue(n, n, nkeys, mismatch=0.001), nkeys)


def test_three_scan_levels(validator):
    """2048 * 2048 + 1 rows: the scans' third level.  Unit adds by two
    processes, a handful of reads at and one below their lower bound."""
    n = SCAN_TILE * SCAN_TILE + 1
    i = np.arange(n)
    op = i // 2
    t = (i % 2).astype(np.uint8)
    f = np.zeros(n, np.uint8)
    p = (op % 2).astype(np.uint32)
    val = np.ones(n, np.int64)
    reads = np.array([3, 1000, SCAN_TILE * 511 + 7, n // 4 - 1, n // 2 - 2])
    for r in reads:
        f[2 * r: 2 * r + 2] = CM.READ
    # an op's lower bound: the ok adds before its invoke = the add ops before it
    lower = reads - np.arange(len(reads))
    val[2 * reads + 1] = lower - (np.arange(len(reads)) % 2)
    val[2 * reads] = CM.NIL
    cols = (t, f, p, val, np.zeros(n, np.uint32))
    got = run_counter(validator, cols, null_key=True)
    assert got["reads"] == len(reads) and got["bad_reads"] == len(reads) // 2
    assert np.array_equal(got["lower"], lower)
    # queue: one value enqueued and dequeued in turn, the last row a surplus dequeue
    fq = (i % 2).astype(np.uint8)
    fq[-1] = CM.DEQ
    res = run_queue(validator, (fq, np.full(n, 9, np.int64), np.zeros(n, np.uint32)), finals=(True,))
    for fifo in (False, True):
        assert res[fifo, True]["error_row"][0] == n - 1


# ---- both entries: keys -------------------------------------------------------
def test_null_key_equals_zero_keys(validator):
    cols = CM.set_reads(CM.gen_counter(5, 700, nkeys=1), 1)
    a = run_counter(validator, cols, 1, null_key=True)
    b = run_counter(validator, cols, 1, null_key=False)
    CM.assert_same(a, b, CM.COUNTER_FIELDS, CM.COUNTER_SCALARS)
    rows = CM.gen_queue(6, 1500, 1)
    a = run_queue(validator, rows, 1, null_key=True)
    b = run_queue(validator, rows, 1, null_key=False)
    for k in a:
        CM.assert_same(a[k], b[k], CM.QUEUE_FIELDS, CM.QUEUE_SCALARS)


def test_more_keys_than_a_tile_holds_rows(validator):
    """5000 keys of a few rows each, key 17 and the last key without rows: the
    key heads and the per-key kernels run over more than one workgroup, and
    key segments straddle every tile edge."""
    nkeys = 5000
    perm = np.arange(nkeys, dtype=np.uint32)
    perm[17] = 4998  # (keys 17 and 4999 get no rows)
    cols = CM.gen_counter(8, 12_000, nprocs=6, nkeys=nkeys - 2, key_perm=perm)
    assert not (cols[4] == 17).any() and not (cols[4] == 4999).any()
    got = run_counter(validator, CM.set_reads(cols, nkeys), nkeys)
    assert got["bad"] > 100 and got["verdict"][17] == 0 and got["read_off"][17] == got["read_off"][18]
    res = run_queue(validator, CM.gen_queue(9, 30_000, nkeys - 2, mismatch=0.01, key_perm=perm), nkeys)
    assert 0 < res[True, True]["bad"] < nkeys and res[False, True]["final_len"][17] == 0


def test_one_malformed_key_among_good_ones(validator):
    """Key 1 of 3 has a double invoke: unknown, no reads listed; its
    neighbours' reads and bounds are what they are without it."""
    cols = list(CM.set_reads(CM.gen_counter(10, 900, nkeys=3), 3, "good"))
    k1 = np.flatnonzero((cols[4] == 1) & (cols[0] == CM.OK))
    cols[0][k1[40]] = CM.INVOKE
    got = run_counter(validator, tuple(cols), 3)
    assert got["verdict"].tolist() == [0, 2, 0] and got["malformed_kind"][1] in (1, 5)
    assert got["read_off"][1] == got["read_off"][2] and got["unknown"] == 1 and got["bad"] == 0
    rows = list(CM.gen_queue(11, 3000, 3, p_enq=0.9))
    k1 = np.flatnonzero((rows[2] == 1) & (rows[0] == CM.DEQ))
    rows[1][k1[5]] = 10 ** 6
    res = run_queue(validator, tuple(rows), 3)
    for fifo in (False, True):
        assert res[fifo, True]["verdict"].tolist() == [0, 1, 0] and res[fifo, True]["error_row"][1] == k1[5]


# ---- both entries: sort paths and buffers -------------------------------------
def test_both_sort_paths(validator):
    """Small ids sort as packed single words; process ids, keys and values
    with 32 / 64 varying bits do not fit beside a row index."""
    cols = CM.set_reads(CM.gen_counter(12, 3000, nkeys=3), 3)
    assert run_counter(validator, cols, 3)["sort_packed"] == 3
    # 32 bits of process, 21 of key, the :info bit and 13 of row index: more than 64
    perm = np.array([0, 0x155555, 0x1FFFFF], np.uint32)
    cols = CM.gen_counter(12, 3000, nkeys=3, proc_mul=0x9E3779B1, key_perm=perm)
    got = run_counter(validator, CM.set_reads(cols, 1 << 21), 1 << 21)
    assert got["sort_packed"] == 2  # (the key sort's rows vary in 21 bits)
    rows = CM.gen_queue(13, 4000, 3)
    res = run_queue(validator, rows, 3, finals=(True,))
    assert res[False, True]["sort_packed"] == 1 and res[True, True]["sort_packed"] == 1
    rows = CM.gen_queue(13, 4000, 3, value_mul=0x0123456789ABCDE)
    res = run_queue(validator, rows, 3, finals=(True,))
    assert res[False, True]["sort_packed"] == 0


def test_buffer_reuse_large_small_large(validator):
    for seed, n, nkeys in ((20, 60_000, 7), (21, 10, 1), (22, 90_000, 300), (23, 6, 2)):
        run_counter(validator, CM.set_reads(CM.gen_counter(seed, n, nkeys=nkeys), nkeys), nkeys)
        run_queue(validator, CM.gen_queue(seed, 2 * n, nkeys, mismatch=0.0005), nkeys)


def test_between_a_resolve_and_its_build(validator):
    v = validator
    h = RM.generated(11, n_txn=800, n_keys=80)
    edges = lambda: [a.copy() for a in v.dep_graph_edges()]  # noqa: E731
    v.dep_graph_resolve(h, arrays=False)
    v.dep_graph_build_resolved(full=True)
    want = edges()
    assert len(want[0]) > 0
    v.dep_graph_resolve(h, arrays=False)
    run_counter(v, CM.set_reads(CM.gen_counter(30, 10_000, nkeys=40), 40), 40)  # more rows than the history has ops
    run_queue(v, CM.gen_queue(31, 20_000, 40), 40)
    v.dep_graph_build_resolved(full=True)
    for x, y in zip(edges(), want):
        np.testing.assert_array_equal(x, y)


def test_interleaved_with_linear_check(validator):
    ops = LM.columns([LM.concurrent_writes(3), LM.concurrent_writes(2, read=9)])
    want = LM.check(ops, None)
    for i in range(3):
        LM.assert_same(validator.linear_check(ops, None), want)
        run_counter(validator, CM.set_reads(CM.gen_counter(40 + i, 400, nkeys=2), 2), 2)
        run_queue(validator, CM.gen_queue(50 + i, 700, 2), 2, finals=(bool(i & 1),))
    LM.assert_same(validator.linear_check(ops, None), want)


# ---- counter ------------------------------------------------------------------
def test_read_and_process_across_tiles(validator):
    """One read invoked in the first scan tile and completed in the third
    (lower gathered from another tile than upper), with an :info row of its
    process in between; then a process of 600 ops, whose sorted rows straddle
    the adjacent-row kernel's workgroup edges."""
    rows = [(CM.INVOKE, CM.READ, 1500, CM.NIL)]
    for p in range(3000):
        rows += [(CM.INVOKE, CM.ADD, p if p < 1500 else p + 1, 2), (CM.OK, CM.ADD, p if p < 1500 else p + 1, 2)]
    rows.insert(1 + 2 * 127, (CM.INFO, CM.OTHER, 1500, CM.NIL))  # an :info row of the reader between the two
    rows.append((CM.OK, CM.READ, 1500, 0))
    got = run_counter(validator, counter_cols(rows))
    assert (got["lower"][0], got["value"][0], got["upper"][0]) == (0, 0, 6000) and got["read_op"][0] == len(rows) - 1
    # a process with 600 ops: its sorted rows straddle workgroup edges
    rows = []
    for i in range(600):
        rows += [(CM.INVOKE, CM.ADD, 3, 1), (CM.INVOKE, CM.READ, 9 + i, CM.NIL), (CM.OK, CM.ADD, 3, 1),
                 (CM.OK, CM.READ, 9 + i, i + 1)]
    got = run_counter(validator, counter_cols(rows))
    assert got["reads"] == 600 and got["bad_reads"] == 0


def test_extremes_wrap_and_inclusive_bounds(validator):
    """int64 extremes, a sum that wraps, reads at lower - 1, lower, upper and
    upper + 1."""
    A, R = CM.ADD, CM.READ
    rows = [(0, A, 0, I64_MAX), (1, A, 0, I64_MAX), (0, A, 1, I64_MAX), (0, R, 2, CM.NIL), (1, R, 2, -2),
            (1, A, 1, 3), (0, A, 0, I64_MIN + 1), (1, A, 0, I64_MIN + 1), (0, R, 2, CM.NIL), (1, R, 2, I64_MAX)]
    got = run_counter(validator, counter_cols(rows))
    assert got["upper"][0] == CM.wrap64(I64_MAX + 3) and got["lower"][0] == I64_MAX
    rows = [(0, A, 0, 5), (1, A, 0, 5), (0, A, 1, 4)]
    for p, val in ((2, 4), (3, 5), (4, 9), (5, 10)):
        rows += [(0, R, p, CM.NIL), (1, R, p, val)]
    got = run_counter(validator, counter_cols(rows))
    assert got["listed_read"].tolist() == [0, 3] and got["errors"][0] == 2 and got["verdict"][0] == 1


def test_more_bad_reads_than_the_list_cap(validator):
    n = hsc.COUNTER_LIST_CAP + 1
    t = np.tile(np.array([CM.INVOKE, CM.OK], np.uint8), n)
    cols = (t, np.full(2 * n, CM.READ, np.uint8), np.zeros(2 * n, np.uint32),
            np.tile(np.array([CM.NIL, 1], np.int64), n), (np.arange(2 * n, dtype=np.uint32) // 2) % 3)
    got = run_counter(validator, cols, 3)
    assert got["bad_reads"] == n and got["n_listed"] == hsc.COUNTER_LIST_CAP and got["errors"].sum() == n


MALFORMED = {
    1: [(0, 0, 0, 1), (0, 0, 0, 1)],
    2: [(0, 0, 0, 1), (1, 0, 0, 1), (1, 0, 0, 1)],
    3: [(0, 0, 0, 1), (2, 0, 0, 2)],
    4: [(0, 0, 0, 1), (1, 1, 0, 1)],
    5: [(0, 1, 0, CM.NIL), (1, 1, 0, CM.NIL)],
}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_each_malformed_kind(validator, kind):
    good = [(0, 0, 7, 1), (1, 0, 7, 1), (0, 1, 8, CM.NIL), (1, 1, 8, 1)]
    rows = good + MALFORMED[kind] + good
    got = run_counter(validator, counter_cols(rows))
    assert got["verdict"][0] == 2 and got["malformed_kind"][0] == kind
    assert got["malformed_op"][0] == len(good) + len(MALFORMED[kind]) - 1 and got["reads"] == 0


def test_two_malformed_kinds_in_one_key(validator):
    """Kind 3 at op 3 and kind 2 at op 1: the smallest index wins, whatever
    its kind; a completion without any predecessor (kind 2, op 0 of key 1)."""
    rows = [(0, 0, 0, 1), (2, 0, 1, 1), (0, 0, 2, 1), (2, 0, 2, 9), (1, 1, 5, 3)]
    got = run_counter(validator, counter_cols(rows, key=[0, 0, 0, 0, 1]), 2)
    assert got["malformed_op"].tolist() == [1, 4] and got["malformed_kind"].tolist() == [2, 2]


def test_random_small_counters_with_malformed(validator):
    """600 keys of at most 16 rows with about 8 % rows of random type in one
    call: the per-key minima and verdicts against the numpy formulation."""
    rng = np.random.default_rng(77)
    nkeys = 600
    n = 6000
    cols = list(CM.gen_counter(78, n // 2, nprocs=3, nkeys=nkeys, differ=0.2, lo_add=-3))
    n = len(cols[0])
    hit = rng.random(n) < 0.02
    cols[0] = np.where(hit, rng.integers(0, 4, n), cols[0]).astype(np.uint8)
    cols[3] = np.where(rng.random(n) < 0.01, CM.NIL, cols[3])
    got = run_counter(validator, CM.set_reads(tuple(cols), nkeys), nkeys)
    assert 20 < got["unknown"] < nkeys - 20 and got["bad"] > 0


# ---- queue --------------------------------------------------------------------
def test_one_value_3000_enqueues_3001_dequeues(validator):
    rows = queue_rows([(CM.ENQ, 4)] * 3000 + [(CM.DEQ, 4)] * 3001)
    res = run_queue(validator, rows)
    assert res[False, True]["error_row"][0] == 6000 and res[True, True]["error_kind"][0] == 2
    res = run_queue(validator, queue_rows([(CM.ENQ, 4)] * 3001 + [(CM.DEQ, 4)] * 3000))
    assert res[False, True]["final_mult"].tolist() == [1] and res[True, True]["final_val"].tolist() == [4]


@pytest.mark.parametrize("at", [0, 255, 256, SCAN_TILE - 1, SCAN_TILE, 2 * SCAN_TILE])
def test_error_at_the_first_row_the_last_row_and_tile_edges(validator, at):
    n = 2 * SCAN_TILE + 1
    f = np.zeros(n, np.uint8)
    val = np.arange(n, dtype=np.int64) % 5
    f[at] = CM.DEQ
    val[at] = 77
    res = run_queue(validator, (f, val, np.zeros(n, np.uint32)), finals=(True,))
    for fifo in (False, True):
        assert res[fifo, True]["error_row"][0] == at and res[fifo, True]["final_len"][0] == 0


def test_fifo_enqueue_in_another_tile_and_which_error_wins(validator):
    """The k-th enqueue 5000 rows before its dequeue; a mismatch before an
    empty dequeue and the other way round."""
    n = 5000
    rows = [(CM.ENQ, i) for i in range(n)] + [(CM.DEQ, i) for i in range(n - 1)] + [(CM.DEQ, n + 5)]
    res = run_queue(validator, queue_rows(rows))
    assert res[True, True]["error_row"][0] == 2 * n - 1 and res[True, True]["error_kind"][0] == 1
    assert res[False, True]["error_kind"][0] == 1
    rows = [(CM.ENQ, 1), (CM.ENQ, 2), (CM.DEQ, 2), (CM.DEQ, 1), (CM.DEQ, 9)]
    res = run_queue(validator, queue_rows(rows))
    assert (res[True, True]["error_row"][0], res[True, True]["error_kind"][0]) == (2, 1)
    assert (res[False, True]["error_row"][0], res[False, True]["error_kind"][0]) == (4, 1)
    rows = [(CM.DEQ, 1), (CM.ENQ, 1), (CM.ENQ, 2), (CM.DEQ, 2)]
    res = run_queue(validator, queue_rows(rows))
    assert (res[True, True]["error_row"][0], res[True, True]["error_kind"][0]) == (0, 2)


def test_queue_int64_extremes_and_final_order(validator):
    rows = queue_rows([(CM.ENQ, I64_MAX), (CM.ENQ, I64_MIN), (CM.ENQ, -1), (CM.ENQ, 0), (CM.ENQ, I64_MIN),
                       (CM.DEQ, I64_MAX)])
    res = run_queue(validator, rows)
    assert res[False, True]["final_val"].tolist() == [I64_MIN, -1, 0]
    assert res[False, True]["final_mult"].tolist() == [2, 1, 1] and res[False, True]["final_len"][0] == 4
    assert res[True, True]["final_val"].tolist() == [I64_MIN, -1, 0, I64_MIN]
    assert res[True, False]["n_final"] == 0 and not res[True, False]["final_off"].any()


# ---- the EDN layer -------------------------------------------------------------
@pytest.mark.parametrize("n_keys", [0, 6])
def test_check_edn_reports(validator, n_keys):
    """The reports of comdb2_amd/jepsen.py from the GPU's dicts equal those
    from the numpy formulation's."""
    ind = n_keys > 0
    text, inj = J.counter_history_edn(60, n_ops=800, n_keys=n_keys, bad_reads=3, malformed=1 if ind else 0)
    got = J.check_counter_edn(validator, text, independent=ind)
    assert got == J.check_counter_edn(ModelValidator(), text, independent=ind) and got["valid"] is False
    text, inj = J.fifo_queue_history_edn(61, n_ops=800, n_keys=n_keys, swap=2)
    for model in ("unordered", "fifo"):
        got = J.check_queue_edn(validator, text, model, independent=ind)
        assert got == J.check_queue_edn(ModelValidator(), text, model, independent=ind)
        assert got["valid"] is (model == "unordered")
    if not ind:  # (a queue history is a counter history without adds or reads)
        rep = J.compose_edn(validator, text, {"queue": J.check_queue_edn, "counter": J.check_counter_edn})
        assert rep["valid"] is True and rep["counter"]["reads"] == []


# ---- the headers' EINVAL cases ---------------------------------------------------
def test_einval(validator):
    v = validator
    one8, one32, one64 = np.zeros(1, np.uint8), np.zeros(1, np.uint32), np.zeros(1, np.int64)

    def counter(n=1, t=one8, f=one8, p=one32, val=one64, key=one32, nkeys=1):
        s = hsc._CounterIn(n, *(None if a is None else a.ctypes.data for a in (t, f, p, val, key)), nkeys)
        return v.lib.hsc_counter_check(v.ctx, C.byref(s), C.byref(hsc.CounterReport()))

    def queue(n=1, f=one8, val=one64, key=one32, nkeys=1, flags=0):
        s = hsc._QueueIn(n, *(None if a is None else a.ctypes.data for a in (f, val, key)), nkeys)
        return v.lib.hsc_queue_check(v.ctx, C.byref(s), flags, C.byref(hsc.QueueReport()))

    assert counter() == hsc.HSC_OK and queue() == hsc.HSC_OK and queue(flags=3) == hsc.HSC_OK
    assert counter(key=None) == hsc.HSC_OK and counter(n=0, t=None, f=None, p=None, val=None, key=None) == hsc.HSC_OK
    for bad in (dict(t=None), dict(f=None), dict(p=None), dict(val=None), dict(nkeys=0), dict(key=None, nkeys=2),
                dict(key=np.ones(1, np.uint32)), dict(key=np.full(1, 5, np.uint32), nkeys=5),
                dict(t=np.full(1, 4, np.uint8)), dict(f=np.full(1, 3, np.uint8)), dict(n=0x80000000)):
        assert counter(**bad) == hsc.HSC_EINVAL, bad
    for bad in (dict(f=None), dict(val=None), dict(nkeys=0), dict(key=None, nkeys=2), dict(key=np.ones(1, np.uint32)),
                dict(f=np.full(1, 2, np.uint8)), dict(flags=4), dict(n=0x80000000)):
        assert queue(**bad) == hsc.HSC_EINVAL, bad
    s = hsc._CounterIn(0, None, None, None, None, None, 1)
    assert v.lib.hsc_counter_check(None, C.byref(s), C.byref(hsc.CounterReport())) == hsc.HSC_EINVAL
    assert v.lib.hsc_counter_check(v.ctx, None, C.byref(hsc.CounterReport())) == hsc.HSC_EINVAL
    assert v.lib.hsc_counter_check(v.ctx, C.byref(s), None) == hsc.HSC_EINVAL
