"""CPU: the model of the set / total-queue / bank checkers (tally_model.py) on
hand-worked answers, the EDN conversions, the report functions, the generators
and the new structs' layouts.  The GPU entries are compared
with this model in test_gpu_tally.py."""
import ctypes
import os
import subprocess
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import tally_model as TM
from comdb2_amd import hsc
from comdb2_amd import jepsen as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- hand-worked answers ----------------------------------------------------
# name: (attempts, acks, final read, valid, ok, lost, unexpected, recovered)
SET_CASES = {
    "all fine": ([0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 3], True, "#{0..3}", "#{}", "#{}", "#{}"),
    "a lost add": ([0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 3], False, "#{0..1 3}", "#{2}", "#{}", "#{}"),
    "never attempted": ([0, 1], [0, 1], [0, 1, 7], False, "#{0..1}", "#{}", "#{7}", "#{}"),
    # 2 completed :info: attempted, not acknowledged, read
    "info recovered": ([0, 1, 2], [0, 1], [0, 1, 2], True, "#{0..2}", "#{}", "#{}", "#{2}"),
    # a set holds a value once however often it was added or read
    "duplicates": ([5, 5, 6, 6, 6], [5, 5, 6], [5, 5, 6], True, "#{5..6}", "#{}", "#{}", "#{}"),
}


@pytest.mark.parametrize("name", sorted(SET_CASES))
def test_set_known_answers(name):
    att, ack, read, valid, ok, lost, unexpected, recovered = SET_CASES[name]
    r = TM.set_checker(att, ack, read)
    assert (r["valid"], r["ok"], r["lost"], r["unexpected"], r["recovered"]) == (valid, ok, lost, unexpected, recovered)
    t = TM.tally(att, ack, read)
    assert t["duplicated"]["count"] == 0 and t["valid"] == int(valid)
    assert t["attempts"] == len(set(att)) and t["acks"] == len(set(ack)) and t["seen"] == len(set(read))


def test_set_never_read():
    assert TM.set_checker([0, 1], [0], None) == {"valid": "unknown", "error": "Set was never read"}
    # an empty read is a read
    r = TM.set_checker([0, 1], [0], [])
    assert r["valid"] is False and r["lost"] == "#{0}" and r["ok"] == "#{}"
    assert r["ok_frac"] == 0 and r["lost_frac"] == Fraction(1, 2)
    assert TM.set_checker([], [], [])["ok_frac"] == 1  # no attempts: unity


# name: (attempts, acks, dequeues, valid, {class: multiset})
QUEUE_CASES = {
    # 4 dequeued twice, enqueued once
    "duplicated": ([3, 4], [3, 4], [3, 4, 4], True,
                   {"ok": {3: 1, 4: 1}, "duplicated": {4: 1}}),
    # 9 was never attempted: both copies are unexpected, none duplicated
    "unexpected twice": ([3], [3], [3, 9, 9], False,
                         {"ok": {3: 1}, "unexpected": {9: 2}}),
    # 5 enqueued twice and acknowledged twice, dequeued once
    "lost once": ([5, 5], [5, 5], [5], False,
                  {"ok": {5: 1}, "lost": {5: 1}}),
    # 7 attempted three times, acknowledged once, dequeued three times
    "recovered": ([7, 7, 7, 8], [7, 8], [7, 7, 7, 8], True,
                  {"ok": {7: 3, 8: 1}, "recovered": {7: 2}}),
}


@pytest.mark.parametrize("name", sorted(QUEUE_CASES))
def test_queue_known_answers(name):
    att, ack, deq, valid, want = QUEUE_CASES[name]
    r = TM.total_queue_checker(att, ack, deq)
    assert r["valid"] is valid
    for c in TM.CLASSES:
        assert r["multisets"][c] == Counter(want.get(c, {})), c
    t = TM.tally(att, ack, deq, multiset=True)
    assert t["attempts"] == len(att) and t["valid"] == int(valid)
    for c in TM.CLASSES:
        assert t[c]["count"] == sum(want.get(c, {}).values())


def test_queue_fractions():
    r = TM.total_queue_checker([7, 7, 7, 8], [7, 8], [7, 7, 7, 8])
    assert r["ok_frac"] == 1 and r["recovered_frac"] == Fraction(1, 2) and r["lost_frac"] == 0


def test_bank_known_answers():
    # wrong-n takes precedence: the short read's sum is wrong too, and is not reported
    reads = [[10, 10, 10], [10, 10], [9, 10, 10], [], [30, -5, 5]]
    r = TM.bank_checker(reads, 3, 30)
    assert r["valid"] is False
    assert r["bad_reads"] == [{"type": "wrong-n", "expected": 3, "found": 2, "op": 1},
                              {"type": "wrong-total", "expected": 30, "found": 29, "op": 2},
                              {"type": "wrong-n", "expected": 3, "found": 0, "op": 3}]
    off = np.cumsum([0] + [len(x) for x in reads])
    b = TM.bank(off, sum(reads, []), 3, 30)
    assert b["kind"].tolist() == [0, 1, 2, 1, 0] and b["found"].tolist() == [30, 2, 29, 0, 30]
    assert b["negatives"].tolist() == [0, 0, 0, 0, 1] and b["reads_with_negative"] == 1
    assert (b["bad"], b["wrong_n"], b["wrong_total"], b["valid"]) == (3, 2, 1, 0)
    # an empty read is fine for a model of no accounts and no money
    assert TM.bank_checker([[]], 0, 0) == {"valid": True, "bad_reads": []}
    # the sum wraps: 2^63 - 1 + 1 is INT64_MIN
    assert TM.bank([0, 2], [TM.INT64_MAX, 1], 2, TM.INT64_MIN)["valid"] == 1


def test_interval_string():
    s = TM.interval_set_str
    assert s([]) == "#{}"
    assert s([4]) == "#{4}"
    assert s([11, 0, 1, 2, 3, 4, 5, 7, 9, 10]) == "#{0..5 7 9..11}"  # util.clj's own example shape
    assert s([-3, -2, -1, 0, 2]) == "#{-3..0 2}"
    assert s([-5, -7]) == "#{-7 -5}"
    assert J.interval_set_str([(0, 5), (7, 7), (9, 11)]) == "#{0..5 7 9..11}"
    assert J.interval_set_str([]) == "#{}" and J.interval_set_str([(-3, 0), (2, 2)]) == "#{-3..0 2}"


def test_runs():
    assert TM.runs_of({1, 2, 3, 5}) == [(1, 3, 1), (5, 5, 1)]
    assert TM.runs_of(Counter({1: 2, 2: 2, 3: 1, 4: 2})) == [(1, 2, 2), (3, 3, 1), (4, 4, 2)]
    assert TM.runs_of({TM.INT64_MIN, TM.INT64_MAX}) == [(TM.INT64_MIN,) * 2 + (1,), (TM.INT64_MAX,) * 2 + (1,)]
    assert TM.runs_of(Counter()) == []


# ---- the EDN conversions ----------------------------------------------------
SET_EDN = """{:type :invoke, :f :add, :value 0, :process 0}
{:type :invoke, :f :add, :value 1, :process 1}
{:type :ok, :f :add, :value 0, :process 0}
{:type :fail, :f :add, :value 1, :process 1}
{:type :invoke, :f :add, :value 2, :process 0}
{:type :info, :f :add, :value 2, :process 0}
{:type :ok, :f :add, :value 3, :process 4}
{:type :invoke, :f :read, :value nil, :process 1}
{:type :ok, :f :read, :value #{0 2}, :process 1}
{:type :invoke, :f :read, :value nil, :process 1}
{:type :ok, :f :read, :value #{0 1 2 9}, :process 1}
"""


def as_vector(text):
    return "[" + text + "]"


def test_set_conversion_counts_as_the_reference():
    for text in (SET_EDN, as_vector(SET_EDN)):
        ops = J.set_ops_from_edn(text)
        # the failed add of 1 is an attempt; the orphan :ok of 3 is an acknowledged add
        assert ops.attempt.tolist() == [0, 1, 2] and ops.ack.tolist() == [0, 3]
        assert ops.seen.tolist() == [0, 1, 2, 9]  # the last :ok :read
        rep = J.set_report(ops, TM.tally(ops.attempt, ops.ack, ops.seen))
        want = TM.set_checker([0, 1, 2], [0, 3], [0, 1, 2, 9])
        assert rep["valid"] is False
        for k in ("ok", "lost", "unexpected", "recovered", "ok_frac", "lost_frac", "unexpected_frac", "recovered_frac"):
            assert rep[k] == want[k], k
        assert (rep["ok"], rep["lost"], rep["unexpected"], rep["recovered"]) == ("#{0..2}", "#{3}", "#{9}", "#{1..2}")
        assert rep["recovered_count"] == 2 and rep["truncated"] == []


def test_set_without_a_read():
    text = "\n".join(SET_EDN.splitlines()[:7])
    ops = J.set_ops_from_edn(text)
    assert ops.seen is None
    assert J.set_report(ops, None) == {"valid": "unknown", "error": "Set was never read"}

    class NoGpu:
        def tally_check(self, *a, **k):
            raise AssertionError("no GPU call without a read")

    assert J.check_set_edn(NoGpu(), text) == {"valid": "unknown", "error": "Set was never read"}


QUEUE_EDN = """{:type :invoke, :f :enqueue, :value 5, :process 0}
{:type :ok, :f :enqueue, :value 5, :process 0}
{:type :invoke, :f :enqueue, :value 5, :process 1}
{:type :info, :f :enqueue, :value 5, :process 1}
{:type :invoke, :f :enqueue, :value 6, :process 0}
{:type :fail, :f :enqueue, :value 6, :process 0}
{:type :invoke, :f :dequeue, :value nil, :process 2}
{:type :ok, :f :dequeue, :value 5, :process 2}
{:type :invoke, :f :dequeue, :value nil, :process 2}
{:type :ok, :f :dequeue, :value 5, :process 2}
{:type :invoke, :f :dequeue, :value nil, :process 2}
{:type :fail, :f :dequeue, :value nil, :process 2}
"""


def test_queue_conversion():
    for text in (QUEUE_EDN, as_vector(QUEUE_EDN)):
        ops = J.queue_ops_from_edn(text)
        assert ops.attempt.tolist() == [5, 5, 6] and ops.ack.tolist() == [5] and ops.seen.tolist() == [5, 5]
        rep = J.total_queue_report(ops, TM.tally(ops.attempt, ops.ack, ops.seen, multiset=True))
        assert rep["valid"] is True and rep["ok"] == [(5, 5, 2)] and rep["recovered"] == [(5, 5, 1)]
        assert rep["lost"] == rep["unexpected"] == rep["duplicated"] == []
        assert rep["ok_frac"] == Fraction(2, 3) and rep["recovered_frac"] == Fraction(1, 3)


BANK_EDN = """{:type :invoke, :f :read, :process 0}
{:type :ok, :f :read, :value [10 10], :process 0}
{:type :invoke, :f :transfer, :value {:from 0, :to 1, :amount 3}, :process 1}
{:type :invoke, :f :read, :process 0}
{:type :ok, :f :read, :value [7 10], :process 0}
{:type :ok, :f :transfer, :value {:from 0, :to 1, :amount 3}, :process 1}
{:type :invoke, :f :read, :process 0}
{:type :fail, :f :read, :process 0}
{:type :invoke, :f :read, :process 0}
{:type :ok, :f :read, :value [7], :process 0}
"""


def test_bank_conversion():
    for text in (BANK_EDN, as_vector(BANK_EDN)):
        ops = J.bank_ops_from_edn(text)
        assert ops.off.tolist() == [0, 2, 4, 5] and ops.balance.tolist() == [10, 10, 7, 10, 7]
        rep = J.bank_report(ops, TM.bank(ops.off, ops.balance, 2, 20), 2, 20)
        assert rep["valid"] is False and rep["bad_read_count"] == 2 and rep["negative_reads"] == 0
        assert [(b["type"], b["expected"], b["found"]) for b in rep["bad_reads"]] == [("wrong-total", 20, 17),
                                                                                    ("wrong-n", 2, 1)]
        assert rep["bad_reads"][0]["op"][":value"] == [7, 10] and rep["bad_reads"][1]["op"] is ops.completions[2]


@pytest.mark.parametrize("text,conv", [
    ("{:type :invoke, :f :add, :value :x, :process 0}", J.set_ops_from_edn),
    ("{:type :ok, :f :add, :value nil, :process 0}", J.set_ops_from_edn),
    ('{:type :ok, :f :read, :value #{1 "a"}, :process 0}', J.set_ops_from_edn),
    ("{:type :ok, :f :dequeue, :value nil, :process 0}", J.queue_ops_from_edn),
    ("{:type :invoke, :f :enqueue, :value [1 2], :process 0}", J.queue_ops_from_edn),
    ("{:type :ok, :f :read, :value [1 true], :process 0}", J.bank_ops_from_edn),
    ("{:type :ok, :f :read, :value nil, :process 0}", J.bank_ops_from_edn),
])
def test_non_integer_values_raise(text, conv):
    with pytest.raises(ValueError):
        conv(text)


# ---- the report functions ---------------------------------------------------
def test_reports_of_a_truncated_class():
    att = list(range(0, 40, 2))  # 20 isolated values, none read: 20 lost runs
    full, cut = TM.tally(att, att, [], multiset=False), TM.tally(att, att, [], multiset=False, cap=3)
    ops = J.TallyOps(np.array(att), np.array(att), np.zeros(0, np.int64))
    rep = J.set_report(ops, cut)
    assert rep["truncated"] == ["lost"] and rep["lost"] == "#{0 2 4}" and rep["lost_count"] == 20
    assert rep["lost_frac"] == 1 and rep["valid"] is False and rep["tally"] is cut
    assert J.set_report(ops, full)["truncated"] == [] and J.set_report(ops, full)["lost"] == TM.interval_set_str(att)
    q = J.total_queue_report(ops, TM.tally(att, att, [], multiset=True, cap=3))
    assert q["truncated"] == ["lost"] and q["lost"] == [(0, 0, 1), (2, 2, 1), (4, 4, 1)] and q["lost_count"] == 20


def test_bank_report_truncated():
    off = np.arange(11)
    res = TM.bank(off, np.ones(10, np.int64), 1, 2, cap=4)
    ops = J.BankOps(off.astype(np.uint64), np.ones(10, np.int64), [{"i": i} for i in range(10)])
    rep = J.bank_report(ops, res, 1, 2)
    assert rep["truncated"] and rep["bad_read_count"] == 10 and [b["op"]["i"] for b in rep["bad_reads"]] == [0, 1, 2, 3]


# ---- the generators ---------------------------------------------------------
def set_model_report(text):
    ops = J.set_ops_from_edn(text)
    return ops, J.set_report(ops, TM.tally(ops.attempt, ops.ack, ops.seen))


SET_GEN = [dict(), dict(lose=3), dict(phantom=4), dict(info_frac=0.2), dict(lose=2, phantom=2, info_frac=0.1)]
QUEUE_GEN = [dict(), dict(lose=3), dict(duplicate=3), dict(unexpected=3), dict(info_frac=0.3),
             dict(lose=2, duplicate=2, unexpected=2, info_frac=0.2)]
BANK_GEN = [dict(), dict(skew_reads=5), dict(short_reads=4), dict(skew_reads=3, short_reads=3)]


@pytest.mark.parametrize("kw", SET_GEN)
def test_set_generator_injections_are_the_findings(kw):
    text, inj = J.set_history_edn(7, n_adds=400, n_procs=5, **kw)
    assert J.set_history_edn(7, n_adds=400, n_procs=5, **kw)[0] == text  # seeded
    _, rep = set_model_report(text)
    for c in ("lost", "unexpected", "recovered", "ok"):
        assert rep[c] == TM.interval_set_str(inj[c]), c
    assert len(inj["lost"]) == kw.get("lose", 0) and len(inj["unexpected"]) == kw.get("phantom", 0)
    assert bool(inj["recovered"]) == bool(kw.get("info_frac"))
    assert rep["valid"] is (not inj["lost"] and not inj["unexpected"])


@pytest.mark.parametrize("kw", QUEUE_GEN)
def test_queue_generator_injections_are_the_findings(kw):
    text, inj = J.queue_history_edn(11, n_enqueues=600, n_procs=5, **kw)
    assert J.queue_history_edn(11, n_enqueues=600, n_procs=5, **kw)[0] == text
    ops = J.queue_ops_from_edn(text)
    chk = TM.total_queue_checker(ops.attempt.tolist(), ops.ack.tolist(), ops.seen.tolist())
    for c in ("lost", "duplicated", "unexpected", "recovered"):
        assert sorted(chk["multisets"][c].items()) == inj[c], c
    assert len(inj["lost"]) == kw.get("lose", 0) and len(inj["duplicated"]) == kw.get("duplicate", 0)
    assert len(inj["unexpected"]) == kw.get("unexpected", 0) and bool(inj["recovered"]) == bool(kw.get("info_frac"))


@pytest.mark.parametrize("kw", BANK_GEN)
def test_bank_generator_injections_are_the_findings(kw):
    n, start = 5, 10
    text, inj = J.bank_history_edn(13, n=n, start=start, n_ops=300, n_procs=4, **kw)
    assert J.bank_history_edn(13, n=n, start=start, n_ops=300, n_procs=4, **kw)[0] == text
    ops = J.bank_ops_from_edn(text)
    rep = J.bank_report(ops, TM.bank(ops.off, ops.balance, n, n * start), n, n * start)
    want = sorted([(r, "wrong-total", n * start - a) for r, a in inj["skewed"]] +
                  [(r, "wrong-n", n - 1) for r in inj["short"]])
    at = {id(op): i for i, op in enumerate(ops.completions)}  # (equal reads are equal dicts)
    got = [(at[id(b["op"])], b["type"], b["found"]) for b in rep["bad_reads"]]
    assert got == want and all(a >= 1 for _, a in inj["skewed"])
    assert len(inj["skewed"]) == kw.get("skew_reads", 0) and len(inj["short"]) == kw.get("short_reads", 0)
    assert rep["negative_reads"] == 0  # the client refuses a transfer that would go negative


# ---- the C ABI --------------------------------------------------------------
def test_struct_layouts_match_header(tmp_path):
    prog = tmp_path / "layout.c"
    prog.write_text("""#include <stdio.h>
#include <stddef.h>
#include "hip_serial.h"
int main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n",
 sizeof(hsc_tally_in), offsetof(hsc_tally_in, seen), sizeof(hsc_tally_class), offsetof(hsc_tally_class, n_listed),
 offsetof(hsc_tally_class, mult), sizeof(hsc_tally_report), offsetof(hsc_tally_report, valid),
 offsetof(hsc_tally_report, cls), offsetof(hsc_tally_report, sort_packed), offsetof(hsc_tally_report, ms),
 sizeof(hsc_bank_in), offsetof(hsc_bank_in, total), sizeof(hsc_bank_report), offsetof(hsc_bank_report, kind),
 offsetof(hsc_bank_report, listed_read), (int)HSC_TALLY_NCLASS, (int)HSC_TALLY_RECOVERED); return 0;}""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(hsc._TallyIn), hsc._TallyIn.seen.offset, ctypes.sizeof(hsc.TallyClass),
            hsc.TallyClass.n_listed.offset, hsc.TallyClass.mult.offset, ctypes.sizeof(hsc.TallyReport),
            hsc.TallyReport.valid.offset, hsc.TallyReport.cls.offset, hsc.TallyReport.sort_packed.offset,
            hsc.TallyReport.ms.offset, ctypes.sizeof(hsc._BankIn), hsc._BankIn.total.offset,
            ctypes.sizeof(hsc.BankReport), hsc.BankReport.kind.offset, hsc.BankReport.listed_read.offset,
            len(hsc.TALLY_CLASSES), hsc.TALLY_CLASSES.index("recovered")]
    assert got == want
    assert hsc.TALLY_CLASSES == TM.CLASSES == J.TALLY_CLASSES
    assert hsc.TALLY_LIST_CAP == hsc.BANK_LIST_CAP == TM.LIST_CAP


def test_host_only_context_has_no_device():
    v = hsc.Validator(-1)
    try:
        with pytest.raises(hsc.HscError, match=r"hsc_tally_check -> -2:"):
            v.tally_check([1], [1], [1])
        with pytest.raises(hsc.HscError, match=r"hsc_bank_check -> -2:"):
            v.bank_check([0, 1], [5], 1, 5)
    finally:
        v.close()


def test_invalid_arguments():
    """HSC_EINVAL comes before the device is asked for: a host-only context shows every case."""
    C = ctypes
    v = hsc.Validator(-1)
    try:
        lib, ctx = v.lib, v.ctx
        one = np.array([1], np.int64)
        ti, tr = hsc._TallyIn(1, 0, 0, one.ctypes.data, None, None), hsc.TallyReport()
        assert lib.hsc_tally_check(ctx, C.byref(ti), 0, C.byref(tr)) == hsc.HSC_EDEVICE
        assert lib.hsc_tally_check(None, C.byref(ti), 0, C.byref(tr)) == hsc.HSC_EINVAL
        assert lib.hsc_tally_check(ctx, None, 0, C.byref(tr)) == hsc.HSC_EINVAL
        assert lib.hsc_tally_check(ctx, C.byref(ti), 0, None) == hsc.HSC_EINVAL
        assert lib.hsc_tally_check(ctx, C.byref(ti), 2, C.byref(tr)) == hsc.HSC_EINVAL  # an unknown flag
        assert lib.hsc_tally_check(ctx, C.byref(ti), 1, C.byref(tr)) == hsc.HSC_EDEVICE
        for bad in (hsc._TallyIn(1, 0, 0, None, None, None), hsc._TallyIn(0, 1, 0, None, None, None),
                    hsc._TallyIn(0, 0, 1, None, None, None),
                    # past the sort's row index: the lengths are checked, the arrays never read
                    hsc._TallyIn(0x80000000, 0, 0, one.ctypes.data, None, None),
                    hsc._TallyIn(0x40000000, 0x40000000, 0, one.ctypes.data, one.ctypes.data, None),
                    hsc._TallyIn(2 ** 64 - 1, 1, 0, one.ctypes.data, one.ctypes.data, None)):
            assert lib.hsc_tally_check(ctx, C.byref(bad), 0, C.byref(tr)) == hsc.HSC_EINVAL

        br = hsc.BankReport()

        def bank(off, bal, nr=None):
            off, bal = np.array(off, np.uint64), np.array(bal, np.int64)
            s = hsc._BankIn(len(off) - 1 if nr is None else nr, off.ctypes.data, bal.ctypes.data, 1, 1)
            return lib.hsc_bank_check(ctx, C.byref(s), C.byref(br))

        assert bank([0, 1, 2], [1, 1]) == hsc.HSC_EDEVICE
        assert bank([1, 2], [1, 1]) == hsc.HSC_EINVAL      # does not start at 0
        assert bank([0, 2, 1], [1, 1]) == hsc.HSC_EINVAL   # descends
        assert bank([0, 1, 1, 2], [1, 1]) == hsc.HSC_EDEVICE  # an empty read is fine
        assert bank([0], [1], nr=0x80000000) == hsc.HSC_EINVAL
        assert bank([0, 2 ** 32], [1]) == hsc.HSC_EINVAL   # more balances than the positions hold
        s = hsc._BankIn(1, None, one.ctypes.data, 1, 1)
        assert lib.hsc_bank_check(ctx, C.byref(s), C.byref(br)) == hsc.HSC_EINVAL
        s = hsc._BankIn(1, np.array([0, 1], np.uint64).ctypes.data, None, 1, 1)
        assert lib.hsc_bank_check(ctx, C.byref(s), C.byref(br)) == hsc.HSC_EINVAL
        assert lib.hsc_bank_check(ctx, None, C.byref(br)) == hsc.HSC_EINVAL
        assert lib.hsc_bank_check(ctx, C.byref(s), None) == hsc.HSC_EINVAL
        assert lib.hsc_bank_check(None, C.byref(s), C.byref(br)) == hsc.HSC_EINVAL
    finally:
        v.close()
