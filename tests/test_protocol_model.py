"""CPU: the verifier of commit-protocol runs (workloads.protocol_replay_check,
the oracle-parity check of bench.py's config-1 protocol leg and
tests/test_gpu_protocol.py).  A sequential run of the protocol is the
commit-stream replay (workloads.replay): rebuilt in the harness's LSN
numbering, the verifier must accept it and reject any flipped verdict."""
import numpy as np

from comdb2_amd.workloads import config1_events, protocol_replay_check, replay


def _sequential_run(events, check, e0=1000):
    """(txns, rc, commit_seq, snap, check_end) of the protocol run by one
    thread in event order: a txn's snapshot has seen the commits before its
    begin, its check the commits before its commit event."""
    txns, idx = [], {}
    for e, t in events:
        if e == "begin":
            idx[t.name] = len(txns)
            txns.append(t)
    n = len(txns)
    rc = np.zeros(n, np.int32)
    seq = np.full(n, -1, np.int64)
    snap = np.zeros(n, np.uint64)
    cend = np.zeros(n, np.uint64)
    rcs = replay(events, check)
    k = 0
    for e, t in events:
        i = idx[t.name]
        if e == "begin":
            snap[i] = e0 + 2 * k
            continue
        if not t.writes:
            continue
        rc[i] = rcs[t.name]
        if rc[i] == 0:
            seq[i] = k
            k += 1
        else:
            cend[i] = e0 + 2 * k
    return txns, rc, seq, snap, cend


def test_harness_checks_a_read_only_txn_only_when_it_holds_a_selectv_array():
    """hsc_harness_commit_protocol's rule for txns without writes, seen on a
    host-only context, whose full checks fail closed (verdict 1): a selectv txn
    with a read set gets its one full check (rc 1 here, the check's end
    recorded), an empty selectv array and a plain read-only txn are never
    checked (db/sqloffload.c:280-287, 505-524); none of them logs anything."""
    from comdb2_amd import formats as F
    from comdb2_amd.hsc import Validator
    from comdb2_amd.workloads import Txn
    k = F.enc_int64(1)
    r = [F.Range("t", 0, k, k)]
    w = [(F.REC_UNDO_UPD_DTA, "t", -2, None), (F.REC_UNDO_UPD_IX, "t", 0, k)]
    txns = [Txn("writer", [], w), Txn("selectv", r, [], True), Txn("selectv_empty", [], [], True),
            Txn("plain", r, [])]
    events = [("begin", t) for t in txns] + [("commit", t) for t in txns]
    v = Validator(-1)
    try:
        v.ingest_log(F.LogBuilder().build())
        rc, seq, snap, cend, st = v.commit_protocol(txns, events, 1)
    finally:
        v.close()
    assert rc.tolist() == [0, 1, 0, 0]
    assert seq.tolist() == [0, -1, -1, -1]
    assert [int(c) != 0 for c in cend] == [False, True, False, False]
    assert (st["commits"], st["aborts"], st["full_checks"]) == (1, 1, 1)


def test_verifier_accepts_a_sequential_run_and_rejects_a_flip(oracle_mod):
    events = config1_events(n_txn=600)
    check = lambda log, rs: oracle_mod.check(log, rs)[0]
    txns, rc, seq, snap, cend = _sequential_run(events, check)
    assert 0 < (rc != 0).sum() < len(rc)
    out = protocol_replay_check(txns, rc, seq, snap, cend, 1000, check)
    assert out["mismatches"] == 0 and out["checked"] == len(txns), out
    # an aborted txn reported as committed by a run that did not commit it
    j = int(np.nonzero(rc != 0)[0][0])
    rc2 = rc.copy()
    rc2[j] = 0
    out = protocol_replay_check(txns, rc2, seq, snap, cend, 1000, check)
    assert out["mismatches"] == 1 and out["first_mismatch"]["txn"] == txns[j].name
    # a snapshot that saw one commit fewer than it did: a later txn that
    # passed now conflicts with a commit it did not see
    flips = 0
    for i in np.nonzero((rc == 0) & (seq > 0))[0][:50]:
        s2 = snap.copy()
        s2[i] = max(1000, int(snap[i]) - 2 * 5)
        flips += protocol_replay_check(txns, rc, seq, s2, cend, 1000, check)["mismatches"]
    assert flips > 0
