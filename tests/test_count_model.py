"""The counter and queue checkers on the CPU: hand-worked pins for both
layers of tests/count_model.py, the numpy formulation of hsc_count.hip's passes
against the line-for-line restatement of the reference on seeded random small
histories, the EDN layer of comdb2_amd/jepsen.py over the numpy formulation,
and the entries' answers on a host-only context."""
import ctypes as C

import numpy as np
import pytest

import count_model as CM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
INV, OK, FAIL, INFO = CM.INVOKE, CM.OK, CM.FAIL, CM.INFO
A, R, O = CM.ADD, CM.READ, CM.OTHER


class ModelValidator:
    """``Validator``'s two methods answered by the numpy formulation."""
    def counter_check(self, type, f, process, value, key=None, nkeys=1):
        return CM.counter_np(type, f, process, value, key, nkeys)

    def queue_check(self, f, value, key=None, nkeys=1, fifo=False, final=False):
        return CM.queue_np(f, value, key, nkeys, fifo=fifo, final=final)


def counter(rows):
    """Both layers on one key's (type, f, process, value) rows; they must
    agree.  -> (valid, reads) or ("unknown", op, kind)."""
    a = np.array(rows, dtype=object).reshape(-1, 4)
    cols = (a[:, 0].astype(np.uint8), a[:, 1].astype(np.uint8), a[:, 2].astype(np.uint32),
            np.array([int(x) for x in a[:, 3]], np.int64))
    got = CM.counter_np(*cols)
    want = CM.counter_plain(CM.rows_of_key(cols, None, 0))
    same_counter(cols, got, want)
    if got["verdict"][0] == CM.V_UNKNOWN:
        return "unknown", int(got["malformed_op"][0]), int(got["malformed_kind"][0])
    return got["verdict"][0] == CM.V_OK, list(zip(got["lower"].tolist(), got["value"].tolist(), got["upper"].tolist()))


def same_counter(cols, got, want):
    """The numpy report of one key against the plain model's.  Where
    history/complete throws, the plain model stops before it looks at values: a
    nil (kind 5) at a smaller op is then the numpy layer's answer alone."""
    if want["valid"] == "unknown":
        assert got["verdict"][0] == CM.V_UNKNOWN and got["reads"] == 0, (cols, got, want)
        mo, mk = int(got["malformed_op"][0]), int(got["malformed_kind"][0])
        if want["phase"] == "loop" or mo == want["op"]:
            assert (mo, mk) == (want["op"], want["kind"]), (cols, got, want)
        else:
            assert mo < want["op"] and mk == 5, (cols, got, want)
        return
    assert got["verdict"][0] == (CM.V_OK if want["valid"] else CM.V_BAD), (cols, got, want)
    assert list(zip(got["lower"].tolist(), got["value"].tolist(), got["upper"].tolist())) == want["reads"]
    assert got["read_op"].tolist() == want["read_ops"]
    assert got["bad_reads"] == len(want["errors"]) == got["errors"][0]
    assert [want["reads"][r] for r in got["listed_read"]] == want["errors"]


def queue(rows, fifo):
    """Both layers on one key's (f, value) rows -> the plain model's report."""
    f = np.array([r[0] for r in rows], np.uint8)
    v = np.array([r[1] for r in rows], np.int64)
    got = CM.queue_np(f, v, fifo=fifo, final=True)
    want = CM.queue_plain([(i, int(f[i]), int(v[i])) for i in range(len(rows))], fifo)
    same_queue(got, want, fifo)
    return want


def same_queue(got, want, fifo):
    if not want["valid"]:
        assert (got["verdict"][0], got["error_row"][0], got["error_kind"][0]) == (CM.V_BAD, want["row"], want["kind"])
        assert got["n_final"] == 0 and got["final_len"][0] == 0
        return
    assert got["verdict"][0] == CM.V_OK and got["error_row"][0] == CM.NO_ROW and got["error_kind"][0] == 0
    fin = got["final_val"].tolist() if fifo else list(zip(got["final_val"].tolist(), got["final_mult"].tolist()))
    assert fin == want["final"]
    assert got["final_len"][0] == (len(fin) if fifo else sum(m for _, m in fin))
    assert got["final_off"].tolist() == [0, len(fin)]


# ---- counter pins -----------------------------------------------------------------
@pytest.mark.parametrize("value,valid", [(0, False), (1, True), (3, True), (4, False)])
def test_a_read_racing_two_adds_has_inclusive_bounds(value, valid):
    rows = [(INV, A, 0, 1), (OK, A, 0, 1), (INV, A, 1, 2), (INV, R, 2, CM.NIL), (OK, A, 1, 2), (OK, R, 2, value)]
    assert counter(rows) == (valid, [(1, value, 3)])


def test_failed_and_info_adds_still_raise_upper():
    for t in (FAIL, INFO):
        rows = [(INV, A, 0, 5), (t, A, 0, 5), (INV, R, 1, CM.NIL), (OK, R, 1, 5)]
        assert counter(rows) == (True, [(0, 5, 5)])


def test_the_completions_value_enters_upper_at_the_invoke():
    rows = [(INV, A, 0, 1), (INV, R, 1, CM.NIL), (OK, R, 1, 7), (OK, A, 0, 7)]
    assert counter(rows) == (True, [(0, 7, 7)])
    rows[3] = (INFO, A, 0, 7)  # (an :info completion fills nothing in)
    assert counter(rows) == (False, [(0, 7, 1)])


def test_negative_increments_and_a_wrapped_sum():
    rows = [(INV, A, 0, -3), (OK, A, 0, -3), (INV, R, 1, CM.NIL), (OK, R, 1, -3)]
    assert counter(rows) == (True, [(-3, -3, -3)])
    rows = [(INV, A, 0, I64_MAX), (OK, A, 0, I64_MAX), (INV, A, 0, 2), (OK, A, 0, 2), (INV, R, 1, CM.NIL),
            (OK, R, 1, I64_MIN + 1)]
    assert counter(rows) == (True, [(I64_MIN + 1, I64_MIN + 1, I64_MIN + 1)])


MALFORMED = {
    1: [(INV, A, 0, 1), (INV, A, 0, 1)],
    2: [(INV, A, 0, 1), (OK, A, 0, 1), (OK, A, 0, 1)],
    3: [(INV, A, 0, 1), (FAIL, A, 0, 2)],
    4: [(INV, A, 0, 1), (OK, R, 0, 1)],
    5: [(INV, R, 0, CM.NIL), (OK, R, 0, CM.NIL)],
}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_each_malformed_kind_and_its_first_offending_op(kind):
    good = [(INV, A, 7, 1), (OK, A, 7, 1), (INFO, O, 0, CM.NIL)]
    rows = good + MALFORMED[kind] + good + MALFORMED[kind]
    assert counter(rows) == ("unknown", len(good) + len(MALFORMED[kind]) - 1, kind)


def test_more_malformed_shapes():
    assert counter([(OK, R, 0, 1)]) == ("unknown", 0, 2)               # no predecessor at all
    assert counter([(INV, A, 0, CM.NIL)]) == ("unknown", 0, 5)          # an add of nil
    assert counter([(INV, A, 0, CM.NIL), (OK, A, 0, 4)]) == (True, [])  # ... that the completion fills in
    assert counter([(INV, A, 0, 4), (OK, A, 0, CM.NIL)]) == ("unknown", 0, 5)
    assert counter([(INV, O, 0, 1), (FAIL, O, 0, 2)]) == ("unknown", 1, 3)  # whatever the f
    assert counter([(INV, A, 0, 1), (INFO, A, 0, 1), (INV, A, 0, 1)]) == ("unknown", 2, 1)  # :info frees nobody


# ---- queue pins -------------------------------------------------------------------
E, D = CM.ENQ, CM.DEQ


def test_a_later_enqueue_repairs_nothing():
    assert queue([(D, 1), (E, 1)], False)["row"] == 0
    got = queue([(D, 1), (E, 1)], True)
    assert (got["row"], got["kind"], got["error"]) == (0, 2, "can't dequeue 1 from empty queue")


def test_the_larger_value_fails_earlier():
    rows = [(E, 5), (D, 9), (D, 5), (D, 5)]
    got = queue(rows, False)
    assert (got["row"], got["error"]) == (1, "can't dequeue 9")
    assert queue([(E, 9), (D, 9), (D, 9), (D, 5)], False)["row"] == 2


def test_fifo_empty_versus_mismatch():
    assert queue([(E, 1), (E, 2), (D, 2)], True)["kind"] == 1
    assert queue([(E, 1), (D, 1), (D, 2)], True)["kind"] == 2
    got = queue([(E, 1), (E, 2), (D, 2), (D, 1), (D, 1), (D, 7)], True)   # the mismatch comes first
    assert (got["row"], got["kind"]) == (2, 1)
    got = queue([(D, 3), (E, 1), (E, 2), (D, 2)], True)                  # the empty one does
    assert (got["row"], got["kind"]) == (0, 2)
    assert queue([(E, 1), (E, 2), (D, 2), (D, 1)], False) == {"valid": True, "final": []}  # legal unordered


def test_an_exact_drain_and_what_is_left():
    assert queue([(E, 1), (E, 2), (D, 1), (D, 2)], True) == {"valid": True, "final": []}
    assert queue([(E, 3), (E, -1), (E, 3), (D, 3)], False) == {"valid": True, "final": [(-1, 1), (3, 1)]}
    assert queue([(E, 3), (E, -1), (E, 3), (D, 3)], True) == {"valid": True, "final": [-1, 3]}


def test_a_failed_enqueue_is_dequeued_legally():
    text = ("{:type :invoke, :f :enqueue, :value 5, :process 0}\n{:type :fail, :f :enqueue, :value 5, :process 0}\n"
            "{:type :invoke, :f :dequeue, :value nil, :process 1}\n{:type :ok, :f :dequeue, :value 5, :process 1}\n"
            "{:type :invoke, :f :dequeue, :value nil, :process 1}\n"
            "{:type :fail, :f :dequeue, :value nil, :process 1}\n")
    for model in ("unordered", "fifo"):
        assert J.check_queue_edn(ModelValidator(), text, model) == {"valid": True, "final_queue": []}


# ---- the numpy formulation against the plain models -----------------------------------
def random_counter(rng):
    """At most 16 ops by 3 processes, about 8 % of random type (and a few nil
    completions), so that a third to a half of the histories are malformed."""
    pend, rows = {}, []
    for _ in range(int(rng.integers(0, 17))):
        p = int(rng.integers(0, 3))
        if rng.random() < 0.08:
            t, f = int(rng.integers(0, 4)), int(rng.integers(0, 3))
            v = CM.NIL if rng.random() < 0.2 else int(rng.integers(-3, 6))
            if t == INV:
                pend[p] = (f, v)
            elif t != INFO:
                pend.pop(p, None)
        elif p in pend:
            f, v = pend[p]
            t = int(rng.choice([OK, OK, OK, FAIL, INFO]))
            if t != INFO:
                del pend[p]
            if t == OK and f != O:
                v = CM.NIL if rng.random() < 0.03 else int(rng.integers(-3, 8))
        else:
            t, f = INV, int(rng.choice([A, A, R, R, O]))
            v = CM.NIL if f == R else int(rng.integers(-3, 6))
            pend[p] = (f, v)
        rows.append((t, f, p, v))
    a = np.array(rows, dtype=np.int64).reshape(-1, 4)
    return a[:, 0].astype(np.uint8), a[:, 1].astype(np.uint8), a[:, 2].astype(np.uint32), a[:, 3]


def test_counter_formulation_equals_the_line_for_line_model():
    rng = np.random.default_rng(1)
    total, malformed = 20_000, 0
    for _ in range(total):
        cols = random_counter(rng)
        want = CM.counter_plain(CM.rows_of_key(cols, None, 0))
        malformed += want["valid"] == "unknown"
        same_counter(cols, CM.counter_np(*cols), want)
    assert 0.3 < malformed / total < 0.6


def test_queue_formulation_equals_the_line_for_line_model():
    rng = np.random.default_rng(2)
    bad = 0
    for _ in range(20_000):
        n = int(rng.integers(0, 15))
        f, v = rng.integers(0, 2, n).astype(np.uint8), rng.integers(0, 3, n).astype(np.int64)
        rows = [(i, int(f[i]), int(v[i])) for i in range(n)]
        for fifo in (False, True):
            want = CM.queue_plain(rows, fifo)
            bad += not want["valid"]
            same_queue(CM.queue_np(f, v, fifo=fifo, final=True), want, fifo)
    assert 10_000 < bad < 36_000


def test_keys_are_judged_independently():
    """Three keys interleaved in one call equal three calls, the plain model
    per independent/subhistory."""
    rng = np.random.default_rng(3)
    for _ in range(300):
        parts = [random_counter(rng) for _ in range(3)]
        key = rng.permutation(np.repeat(np.arange(3, dtype=np.uint32), [len(p[0]) for p in parts]))
        cols = [np.empty(len(key), p.dtype) for p in parts[0]]
        for k, part in enumerate(parts):
            for c, src in zip(cols, part):
                c[key == k] = src
        got = CM.counter_np(*cols, key, 3)
        hist = [{"index": i, "type": int(cols[0][i]), "f": int(cols[1][i]), "process": int(cols[2][i]),
                 "value": (int(key[i]), int(cols[3][i]))} for i in range(len(key))]
        for k, part in enumerate(parts):
            one = CM.counter_np(*part)
            assert got["verdict"][k] == one["verdict"][0] and got["errors"][k] == one["errors"][0]
            a, b = got["read_off"][k], got["read_off"][k + 1]
            assert got["lower"][a:b].tolist() == one["lower"].tolist()
            assert got["upper"][a:b].tolist() == one["upper"].tolist()
            want = CM.counter_plain(CM.subhistory(k, hist))
            assert (want["valid"] == "unknown") == (got["verdict"][k] == CM.V_UNKNOWN)
            if want["valid"] != "unknown":
                assert want["read_ops"] == got["read_op"][a:b].tolist()


# ---- the EDN layer ---------------------------------------------------------------
def test_check_counter_edn():
    mv = ModelValidator()
    text, inj = J.counter_history_edn(5, n_ops=300)
    rep = J.check_counter_edn(mv, text)
    assert rep["valid"] is True and len(rep["reads"]) > 50 and rep["errors"] == []
    assert all(lo <= v <= hi for lo, v, hi in rep["reads"])
    text, inj = J.counter_history_edn(5, n_ops=300, bad_reads=3)
    rep = J.check_counter_edn(mv, text)
    assert rep["valid"] is False and len(rep["errors"]) == 3 and all(v == hi + 1 for _, v, hi in rep["errors"])
    text, inj = J.counter_history_edn(5, n_ops=300, malformed=1)
    rep = J.check_counter_edn(mv, text)
    assert rep["valid"] == "unknown" and rep["kind"] == 2 and "malformed history at op" in rep["error"]
    assert rep["op"][":type"] in (":ok", ":fail")


def test_check_counter_edn_independent():
    mv = ModelValidator()
    text, inj = J.counter_history_edn(6, n_ops=900, n_keys=7, bad_reads=4, malformed=2)
    # (an un-keyed :info op is in every subhistory and changes nothing)
    text += "{:type :info, :f :start, :value nil, :process :nemesis}\n"
    rep = J.check_counter_edn(mv, text, independent=True)
    assert set(rep["results"]) == set(range(7)) and inj["malformed"] and inj["bad"]
    for k, r in rep["results"].items():
        want = "unknown" if k in inj["malformed"] else False if k in inj["bad"] else True
        assert r["valid"] is want or r["valid"] == want, (k, r["valid"], want)
    assert rep["valid"] is False and sorted(rep["failures"]) == sorted(set(inj["bad"]) | set(inj["malformed"]))
    with pytest.raises(ValueError, match="un-keyed"):
        J.check_counter_edn(mv, text + "{:type :invoke, :f :read, :value nil, :process 99}\n", independent=True)


@pytest.mark.parametrize("n_keys", [0, 5])
def test_check_queue_edn(n_keys):
    mv = ModelValidator()
    ind = n_keys > 0
    one = (lambda r: r["results"]) if ind else (lambda r: {0: r})
    text, _ = J.fifo_queue_history_edn(7, n_ops=500, n_keys=n_keys)
    for model in ("unordered", "fifo"):
        rep = J.check_queue_edn(mv, text, model, independent=ind)
        assert rep["valid"] is True and all(r["valid"] is True for r in one(rep).values())
    fin_u, fin_f = (one(J.check_queue_edn(mv, text, m, independent=ind)) for m in ("unordered", "fifo"))
    for k in fin_u:
        assert sorted(fin_f[k]["final_queue"]) == [v for v, m in fin_u[k]["final_queue"] for _ in range(m)]
    text, inj = J.fifo_queue_history_edn(7, n_ops=500, n_keys=n_keys, swap=2)
    assert J.check_queue_edn(mv, text, "unordered", independent=ind)["valid"] is True
    rep = J.check_queue_edn(mv, text, "fifo", independent=ind)
    assert rep["valid"] is False and inj["swapped"]
    assert sorted(k for k, r in one(rep).items() if not r["valid"]) == inj["swapped"]
    assert all(r["error"].startswith("can't dequeue ") for r in one(rep).values() if not r["valid"])
    text, inj = J.fifo_queue_history_edn(7, n_ops=500, n_keys=n_keys, phantom=1)
    for model in ("unordered", "fifo"):
        rep = J.check_queue_edn(mv, text, model, independent=ind)
        assert rep["valid"] is False and (not ind or rep["failures"] == inj["phantom"])


def test_compose_with_the_new_members():
    mv = ModelValidator()
    text, _ = J.counter_history_edn(8, n_ops=200, bad_reads=1)
    rep = J.compose_edn(mv, text, {"counter": J.check_counter_edn, "queue": J.check_queue_edn})
    assert rep["counter"]["valid"] is False and rep["queue"] == {"valid": True, "final_queue": []}
    assert rep["valid"] is False
    text, _ = J.counter_history_edn(8, n_ops=200, malformed=1)
    assert J.compose_edn(mv, text, {"counter": J.check_counter_edn})["valid"] == "unknown"
    text, _ = J.fifo_queue_history_edn(9, n_ops=200, n_keys=3)
    rep = J.compose_edn(mv, text, {"queue": lambda v, t: J.check_queue_edn(v, t, "fifo", independent=True)})
    assert rep["valid"] is True and set(rep["queue"]["results"]) == {0, 1, 2}


def test_generators_keep_their_output():
    """The generators added for these checkers are functions of their
    arguments (and the older ones do not share their random streams)."""
    assert J.counter_history_edn(3, 50) == J.counter_history_edn(3, 50)
    assert J.fifo_queue_history_edn(3, 50, n_keys=2) == J.fifo_queue_history_edn(3, 50, n_keys=2)


# ---- the C ABI on a host-only context -------------------------------------------------
def test_host_only_context_has_no_device():
    v = hsc.Validator(-1)
    try:
        with pytest.raises(hsc.HscError, match=r"hsc_counter_check -> -2:"):
            v.counter_check([0], [0], [0], [1])
        with pytest.raises(hsc.HscError, match=r"hsc_queue_check -> -2:"):
            v.queue_check([0], [1])
        # the arguments are checked first, as hsc_tally_check does
        one8, one32, one64 = np.zeros(1, np.uint8), np.ones(1, np.uint32), np.zeros(1, np.int64)
        s = hsc._CounterIn(1, one8.ctypes.data, one8.ctypes.data, one32.ctypes.data, one64.ctypes.data,
                           one32.ctypes.data, 1)  # key 1 of 1
        assert v.lib.hsc_counter_check(v.ctx, C.byref(s), C.byref(hsc.CounterReport())) == hsc.HSC_EINVAL
        q = hsc._QueueIn(1, one8.ctypes.data, one64.ctypes.data, None, 1)
        assert v.lib.hsc_queue_check(v.ctx, C.byref(q), 4, C.byref(hsc.QueueReport())) == hsc.HSC_EINVAL
        assert v.lib.hsc_queue_check(v.ctx, C.byref(q), 3, C.byref(hsc.QueueReport())) == hsc.HSC_EDEVICE
        s = hsc._CounterIn(0, None, None, None, None, None, 1)
        assert v.lib.hsc_counter_check(v.ctx, C.byref(s), C.byref(hsc.CounterReport())) == hsc.HSC_EDEVICE
    finally:
        v.close()
