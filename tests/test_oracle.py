"""CPU: pin the oracle (C restatement of bdb_osql_serial_check) against the
reference's own known answers (tests/serialstep.test, restated in
tests/golden/serialstep.json; tests/selectv_range.test and
tests/selectv_recom_range.test, restated in tests/golden/selectv_range.json)
and against an independent set-formula model."""
import numpy as np
import pytest

from comdb2_amd import formats as F
from comdb2_amd.formats import LogBuilder, Range, ReadSets
from comdb2_amd.workloads import Txn, config1_events, config2, random_case, replay
from helpers import (commit_verdicts, model_check, scenario_events, selectv_cases, selectv_events,
                     selectv_range, serialstep)


def oracle_checker(o):
    return lambda log, rs: o.check(log, rs)[0]


@pytest.mark.parametrize("name", sorted(serialstep()))
def test_serialstep_known_answers(oracle_mod, name):
    sc = serialstep()[name]
    rcs = replay(scenario_events(sc), oracle_checker(oracle_mod))
    failed = sorted(t for t, rc in rcs.items() if rc)
    assert failed == sorted(sc["expect_fail"])
    assert len(failed) == sc["reference_failures"]


def test_serialstep_model_agrees():
    for name, sc in serialstep().items():
        rcs = replay(scenario_events(sc), lambda log, rs: model_check(log, rs)[0])
        assert sorted(t for t, rc in rcs.items() if rc) == sorted(sc["expect_fail"]), name


SELECTV = [pytest.param(sc, id=f"{name}-{vname}") for name, vname, sc in selectv_cases()]


@pytest.fixture(scope="module")
def host_checker():
    """The host path of DESIGN §5c as a checker.  A host-only context refuses
    check_readsets (tests/test_marshal.py), so the verdict is the native
    marshaller's forced verdicts or'ed with the probe-level model of the join
    over the batch it marshalled."""
    from comdb2_amd.hsc import Validator
    from probe_model import WindowModel, evaluate
    v = Validator(-1)

    def check(log, rs):
        v.ingest_log(log)
        m = v.marshal(rs)
        return (evaluate(v, m, WindowModel(log)) | m["forced"]) != 0
    yield check
    v.close()


def selectv_checkers(oracle_mod, host_checker):
    return {"oracle": oracle_checker(oracle_mod), "model": lambda log, rs: model_check(log, rs)[0],
            "host": host_checker}


@pytest.mark.parametrize("sc", SELECTV)
def test_selectv_range_known_answers(oracle_mod, host_checker, sc):
    """tests/golden/selectv_range.json: the ordered commit verdicts of every
    scenario and variant equal the reference's, by the C oracle, the set-formula
    model and the host path; with the read set as captured and coalesced
    (oracle/coalesce_oracle.c); with the snapshot at begin (the reference's) and
    just after the txn's last read."""
    for who, check in selectv_checkers(oracle_mod, host_checker).items():
        for form in ("raw", "coalesced"):
            chk = check if form == "raw" else (lambda log, rs, c=check: c(log, oracle_mod.coalesce(rs)))
            for snapshot in ("begin", "last_read"):
                rcs = replay(selectv_events(sc, snapshot), chk)
                assert commit_verdicts(sc, rcs) == sc["reference_commits"], (who, form, snapshot, rcs)
                # what was checked: every selectv txn with a read set, and every write txn
                want = {n for n, t in sc["txns"].items() if t["writes"] or (t["selectv"] and t["reads"])}
                assert set(rcs) == want, (who, form, snapshot)


def test_selectv_range_fixture_shape():
    """20 commits, 10 failing; every situation the issue names is present."""
    cases = selectv_range()
    commits = [v for sc in cases.values() for v in sc["reference_commits"]]
    assert (len(commits), sum(commits)) == (20, 10)
    for name, sc in cases.items():
        assert len(sc["commits"]) == len(sc["reference_commits"]), name
        assert sc["reference_commits"] == [int(n in sc["expect_fail"]) for n in sc["commits"]], name
    txns = [(n, t) for sc in cases.values() for n, t in sc["txns"].items()]
    assert any(t["selectv"] and t["reads"] and not t["writes"] for _, t in txns)   # read-only, checked
    assert any(not t["selectv"] and not t["reads"] and not t["writes"] for _, t in txns)  # never checked
    keyless = cases["range.t5_08"]["txns"]["B1"]["writes"]
    assert [w[0] for w in keyless] == ["upd_dta"]                                   # a data record only


@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_selectv_matrix_verdicts_hold_by_construction(oracle_mod, host_checker, kind):
    """tests/selectv_matrix.py at a small tile size: the filler changes no
    scenario verdict and every decoy's verdict is the constructed one -- by
    the oracle, the model (one offset) and the host path."""
    import selectv_matrix as M
    windows = M.build(64, kind)
    assert len(windows) == 3 * 24                   # 24 checked commits over all variants, 3 offsets
    for i, w in enumerate(windows):
        assert w.pool.ntxn == M.POOL and w.want[1:].any() and not w.want[1:].all()
        np.testing.assert_array_equal(oracle_mod.check(w.log, w.pool)[0] != 0, w.want,
                                      err_msg=f"oracle: {w.what}")
        np.testing.assert_array_equal(host_checker(w.log, w.pool), w.want, err_msg=f"host: {w.what}")
        if i % 3 == 0:
            np.testing.assert_array_equal(model_check(w.log, w.pool)[0] != 0, w.want,
                                          err_msg=f"model: {w.what}")
    # 10 failing commits, and the second variants of recom.t5_01 (1) and recom.t6_01 (3) again
    assert sum(w.want[0] for w in windows) == 3 * 14
    sizes = [(n, p) for (n, p), _ in windows[0].batches()]
    assert len(sizes) == 12 and all(idx[p] == 0 and len(idx) == n and len(set(idx)) == n
                                    for (n, p), idx in windows[0].batches())


def test_replay_checks_read_only_selectv_only():
    """replay's rule: a txn without writes is checked iff it is a selectv txn
    with a read set; nothing it 'commits' reaches the log."""
    k = F.enc_int64(1)
    r = [Range("t", 0, k, k)]
    w = [(F.REC_UNDO_UPD_DTA, "t", -2, None), (F.REC_UNDO_UPD_IX, "t", 0, k)]
    seen = []

    def check(log, rs):
        seen.append((log.nrec, rs.nranges))
        return model_check(log, rs)[0]
    for selectv, reads, checked in ((False, r, False), (True, [], False), (True, r, True)):
        ro, wr = Txn("ro", reads, [], selectv), Txn("w", [], w)
        ev = [("begin", ro), ("begin", wr), ("commit", wr), ("commit", ro)]
        del seen[:]
        rcs = replay(ev, check)
        assert rcs == ({"w": 0, "ro": 1} if checked else {"w": 0}), (selectv, reads)
        assert len(seen) == (2 if checked else 1)
        # the read-only txn passing (snapshot after the write) logs nothing
        ev = [("begin", wr), ("commit", wr), ("begin", ro), ("commit", ro), ("begin", ro), ("commit", ro)]
        del seen[:]
        rcs = replay(ev, check)
        assert rcs == ({"w": 0, "ro": 0} if checked else {"w": 0})
        if checked:
            assert seen[1][0] == seen[2][0] > seen[0][0]             # the log did not grow


@pytest.mark.parametrize("seed", range(12))
def test_oracle_vs_model_random(oracle_mod, seed):
    log, rs = random_case(seed, broken=(seed % 3 == 0))
    for regop_only in (0, 1):
        rc, post, _ = oracle_mod.check(log, rs, regop_only=regop_only)
        mrc, mpost = model_check(log, rs, regop_only=regop_only)
        np.testing.assert_array_equal(rc != 0, mrc != 0)
        np.testing.assert_array_equal(post, mpost)


def _one(oracle_mod, lb, ranges, snap, regop_only=0):
    log = lb.build()
    rs = ReadSets.from_lists([ranges], [snap], tbnames=lb.tbnames)
    rc, post, _ = oracle_mod.check(log, rs, regop_only=regop_only)
    return int(rc[0] != 0), int(post[0]), log


def test_min_length_memcmp_prefix(oracle_mod):
    lb = LogBuilder(["t"])
    s = lb.next_lsn()
    lb.begin(1)
    lb.write(1, F.REC_UNDO_UPD_IX, "t", 0, F.enc_int64(5) + F.enc_int64(7))
    lb.commit(1)
    pre = F.enc_int64(5)
    assert _one(oracle_mod, lb, [Range("t", 0, pre, pre)], s)[0] == 1        # prefix hit
    assert _one(oracle_mod, lb, [Range("t", 0, F.enc_int64(6), None, 0, 1)], s)[0] == 0
    long_lo = F.enc_int64(5) + F.enc_int64(7) + b"\xff"                        # longer than key
    assert _one(oracle_mod, lb, [Range("t", 0, long_lo, long_lo)], s)[0] == 1  # truncated compare
    assert _one(oracle_mod, lb, [Range("t", 0, b"", b"")], s)[0] == 1          # zero-length bounds
    assert _one(oracle_mod, lb, [Range("t", 1, pre, pre)], s)[0] == 0          # other index


def test_span_quirk_and_first_range_lock(oracle_mod):
    lb = LogBuilder(["a", "b"])
    s = lb.next_lsn()
    lb.begin(1)
    lb.write(1, F.REC_UNDO_ADD_IX_LK, "a", 0, F.enc_int64(10))
    lb.write(1, F.REC_UNDO_DEL_DTA, "a")
    lb.commit(1)
    k = F.enc_int64
    # a's ix0 span covers array slots 0..2, including b's range [10,10]
    unsorted = [Range("a", 0, k(5), k(5)), Range("b", 0, k(10), k(10)), Range("a", 0, k(7), k(7))]
    assert _one(oracle_mod, lb, unsorted, s)[0] == 1
    assert _one(oracle_mod, lb, [unsorted[0], unsorted[2], unsorted[1]], s)[0] == 0
    # islocked comes from the table's FIRST range: a later locked range is ignored
    assert _one(oracle_mod, lb, [Range("a", 1, k(0), k(0)), Range.locked("a")], s)[0] == 0
    assert _one(oracle_mod, lb, [Range.locked("a"), Range("a", 1, k(0), k(0))], s)[0] == 1


def test_window_rules(oracle_mod):
    lb = LogBuilder(["t"])
    s0 = lb.next_lsn()
    k = F.enc_int64(1)
    lb.begin(1)
    lb.write(1, F.REC_UNDO_UPD_IX, "t", 0, k)
    lb.commit(1, isabort=1)                       # aborted: ignored
    lb.commit(2, empty=True)                      # read-only logical txn: ignored
    st = lb.begin(3)
    lb.raw(F.REC_TXN_REGOP, prev=st)              # regop not pointing at a commit
    r = [Range("t", 0, k, k)]
    rc, post, log = _one(oracle_mod, lb, r, s0)
    assert rc == 0 and post == int(log.end_lsn)   # full mode moves the LSN to the end
    assert _one(oracle_mod, lb, r, s0, regop_only=1)[:2] == (0, s0)
    lb.begin(4)
    lb.write(4, F.REC_UNDO_UPD_IX, "t", 0, k)
    c4 = lb.commit(4)
    assert _one(oracle_mod, lb, r, s0)[0] == 1
    assert _one(oracle_mod, lb, r, c4)[0] == 0    # snapshot at the commit itself
    assert _one(oracle_mod, lb, [], s0)[0] == 0   # empty read set never conflicts
    assert _one(oracle_mod, lb, r, s0, regop_only=1)[0] == 1
    end = int(lb.build().end_lsn)
    assert _one(oracle_mod, lb, r, end)[0] == 0   # at end of log: DB_NOTFOUND -> 0
    assert _one(oracle_mod, lb, r, s0 + 1)[0] == 1  # not a record LSN: cursor error


def test_config1_replay_small(oracle_mod):
    ev = config1_events(n_txn=200)
    rcs = replay(ev, oracle_checker(oracle_mod))
    mrcs = replay(ev, lambda log, rs: model_check(log, rs)[0])
    assert rcs == mrcs
    assert 0 < sum(rcs.values()) < len(rcs)


def test_config2_small_oracle_vs_model(oracle_mod):
    c2 = config2(n_commits=300, n_txn=60, value_bits=16, width=1 << 8, snap_recent=0.5)
    rc, _, _ = oracle_mod.check(c2.log, c2.readsets)
    mrc, _ = model_check(c2.log, c2.readsets)
    np.testing.assert_array_equal(rc != 0, mrc != 0)
