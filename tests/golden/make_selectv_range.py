"""Generate tests/golden/selectv_range.json: the reference's SELECTV range
known-answer tests (tests/selectv_range.test and tests/selectv_recom_range.test,
the batches driven by tests/tools/stepper.c, plus the single-session t3_03)
restated as read sets + write sets at the level bdb_osql_serial_check sees them.

Run where the reference is readable (it walks every .req beside its .req.out
to record, commit by commit, whether the commit failed with "selectv
constraints"; the committed JSON is all the tests need):
    python tests/golden/make_selectv_range.py

Why that string is a verdict of the check: only db/sqloffload.c:301-311
(osql_sock_commit), db/sqloffload.c:518-523 (selectv_range_commit) and
db/toblock.c:4802-4816 produce it, each from bdb_osql_serial_check(...,
regop_only = 0) on clnt->selectv_arr / iq->selectv_arr.

Restatement rules (how the SQL becomes CurRange's and logged records):
  * only recording cursors feed selectv_arr: a closing or re-seeking cursor
    appends its range to clnt->selectv_arr iff pCur->is_recording, and only
    inside a transaction (db/sqlglue.c:3468-3477, 3723-3732, 5952-5961,
    9170-9179); a cursor records iff its SELECT was a selectv
    (sqlite/select.c:4501, 5906-5908 -> OP_OpenRead_Record, sqlite/vdbe.c:
    3982-3983 -> sqlite3BtreeSetRecording, db/sqlglue.c:10104-10120).  So a
    plain select -- a `select count(*)`, the plain arm of a UNION, an
    `insert ... select` -- captures nothing, and neither does the cursor an
    update or delete statement opens for itself inside a selectv transaction;
    of a UNION of a selectv and a select only the selectv arm's table is
    captured (range t5_03 / t5_04 / t5_05 decide this: see below);
  * a full scan is a table lock: First sets lflag (db/sqlglue.c:3747), Next
    running off the end sets rflag (8381-8387), and both flags make islocked
    (8399-8400); on the data file (ixnum -1) First locks at once (3753-3754);
  * a table with no index has only the data file, ixnum -1: a scan of it is
    a table lock (db/sqlglue.c:3753-3754, 8367-8370);
  * a filter no index can serve (`id % 2 = 0`) scans the whole table: a lock;
  * `id < v` where every row qualifies runs off the end like a full scan
    (reading "ran_off_end": a lock); the other reading keeps the bound,
    (open, k(v)] (make_serialstep's rule for `id < v`).  Both are kept;
  * `id > a and id < b`: the seek stores the searched key as lkey
    (db/sqlglue.c:9201-9203) and, the found row being greater, that row's key
    as rkey (9290-9296); every Next moves rkey to the row it lands on
    (8388-8397), the row that fails `id < b` included.  Reading "stop_row":
    [k(a), k(stop row)]; reading "bound": [k(a), k(b)].  Both are kept; the
    check compares both ends closed;
  * a point lookup on the unique index finds its key: lkey = rkey = k
    (db/sqlglue.c:9201-9203, 9229-9232) and no Next follows -- range t2_01's
    second commit passes while the next row (id 2) is deleted, which a range
    stretched to the next row would not;
  * the snapshot is taken when the transaction begins (db/sqlglue.c:4512-4525
    -> get_current_lsn, 4293-4309); the array is coalesced before the commit
    (db/sqlglue.c:4602-4603);
  * a selectv transaction is checked at commit even when it wrote nothing
    (db/sqlglue.c:4688-4689 -> selectv_range_commit, db/sqloffload.c:505-524),
    unless its array is empty (510-514); a transaction with no selectv has an
    empty array and is never checked for selectv constraints;
  * an update of non-key columns logs upd_dta + upd_ix of every index key of
    the row (bdb/ll.c:749, as make_serialstep); a key change upd_dta +
    del_ix(old) + add_ix(new); insert add_dta + add_ix; delete del_dta +
    del_ix; on the keyless t2 (selectv_range.test/t2.csc2 has no keys
    section) only the data record;
  * t1.id is a 4-byte int: make_serialstep.enc_int32 is its key;
  * session 1's statements outside a transaction are autocommit writes that
    are never checked (the A* txns, as A1 of serialstep s14);
  * tables persist across cases or are truncated as the .fastinit files say:
    selectv_range t2 truncates t1 and t2, t5 truncates t2 only (t1 keeps the
    seven rows id 1..7 that t5_01's final count and the UNION outputs show);
    selectv_recom_range truncates both before t2, t5 and t6.

The JSON holds no statement of the .req files and no line of their outputs:
each statement is described in the comments below in this file's own words.
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_serialstep import enc_int32, locked, rng_  # noqa: E402

REF = "/root/reference/tests"
FAILED = re.compile(r"selectv constraints")

k = enc_int32


def ins1(i):
    return [("add_dta", "t1", -2, None), ("add_ix", "t1", 0, k(i).hex())]


def del1(i):
    return [("del_dta", "t1", -2, None), ("del_ix", "t1", 0, k(i).hex())]


def upd1(i):
    """non-key update of t1 row i (also a key update that leaves the key as it is)"""
    return [("upd_dta", "t1", -2, None), ("upd_ix", "t1", 0, k(i).hex())]


def mov1(a, b):
    return [("upd_dta", "t1", -2, None), ("del_ix", "t1", 0, k(a).hex()), ("add_ix", "t1", 0, k(b).hex())]


def point(i):
    return rng_("t1", 0, k(i), k(i))


def auto(writes):
    return dict(reads=[], writes=writes, selectv=False)


def sv(reads, writes=()):
    return dict(reads=reads, writes=list(writes), selectv=True)


def plain(writes=()):
    """a transaction without a selectv: no read set"""
    return dict(reads=[], writes=list(writes), selectv=False)


def seq(*steps):
    """events from (kind, txn) steps; an autocommit txn is ('auto', name)."""
    ev = []
    for kind, name in steps:
        if kind == "auto":
            ev += [["begin", name], ["commit", name]]
        else:
            ev.append([kind, name])
    return ev


def scenarios():
    out = {}
    T2_KEYLESS_UPD = [("upd_dta", "t2", -2, None)]

    # t2_01 (the same statements in both directories): session 1 inserts row
    # 1; T1 scans all of t1 (lock) and session 1 deletes row 1 -> fail; rows
    # 1 and 2 are inserted; T2 looks up id 1 and session 1 deletes row 2 ->
    # pass.  Both transactions are read-only.
    def t2_01():
        return dict(
            txns={"A1": auto(ins1(1)), "T1": sv([locked("t1")]), "A2": auto(del1(1)),
                  "A3": auto(ins1(1)), "A4": auto(ins1(2)), "T2": sv([point(1)]), "A5": auto(del1(2))},
            events=seq(("auto", "A1"), ("begin", "T1"), ("read", "T1"), ("auto", "A2"), ("commit", "T1"),
                       ("auto", "A3"), ("auto", "A4"), ("begin", "T2"), ("read", "T2"), ("auto", "A5"),
                       ("commit", "T2")),
            commits=["T1", "T2"], expect_fail=["T1"], variants={"as_read": {}})

    out["range.t2_01"] = dict(t2_01(), reference_file="selectv_range.test/t2_01.req")
    out["recom.t2_01"] = dict(t2_01(), reference_file="selectv_recom_range.test/t2_01.req")

    # range t3_03, one session: three transactions each scan the keyless t2
    # with a selectv (lock) after a plain count, then insert a row, update it,
    # delete it.  Nobody else writes: all pass.
    out["range.t3_03"] = dict(
        txns={"T1": sv([locked("t2")], [("add_dta", "t2", -2, None)]),
              "T2": sv([locked("t2")], T2_KEYLESS_UPD),
              "T3": sv([locked("t2")], [("del_dta", "t2", -2, None)])},
        events=seq(("begin", "T1"), ("read", "T1"), ("commit", "T1"), ("begin", "T2"), ("read", "T2"),
                   ("commit", "T2"), ("begin", "T3"), ("read", "T3"), ("commit", "T3")),
        commits=["T1", "T2", "T3"], expect_fail=[], variants={"as_read": {}},
        reference_file="selectv_range.test/t3_03.req")

    # range t5_*: t1 holds rows 1..7, t2 (keyless) is empty before t5_01 and
    # holds 1..7 after it.  Session 2's write is a blob update of t1 row 1
    # (B1) or a move of t2's id 1 -> 111 (B2, a data record only).
    seven = [("add_dta", "t2", -2, None)] * 7
    # t5_01: T1 inserts into t2 what a selectv scan of t1 returns (lock t1),
    # session 2 updates t1 row 1 -> fail; T2 does the same with a plain
    # select: no read set, unchecked, its seven rows go in.
    out["range.t5_01"] = dict(
        txns={"T1": sv([locked("t1")], seven), "B1": auto(upd1(1)),
              "T2": plain(seven), "B2": auto(upd1(1))},
        events=seq(("begin", "T1"), ("read", "T1"), ("auto", "B1"), ("commit", "T1"),
                   ("begin", "T2"), ("auto", "B2"), ("commit", "T2")),
        commits=["T1", "T2"], expect_fail=["T1"], variants={"as_read": {}},
        reference_file="selectv_range.test/t5_01.req")

    def union(reads, other, restore=False):
        txns = {"T1": sv(reads) if reads else plain(), "B1": auto(other)}
        ev = [("begin", "T1")] + ([("read", "T1")] if reads else []) + [("auto", "B1"), ("commit", "T1")]
        if restore:  # session 2 moves t2's row back afterwards
            txns["B2"] = auto(T2_KEYLESS_UPD)
            ev.append(("auto", "B2"))
        return txns, seq(*ev)

    # (case, the UNION's selectv arms, session 2's write, verdict)
    for case, arms, other, fails, restore in (
            ("t5_02", [], upd1(1), False, False),                  # no selectv at all
            ("t5_03", ["t1"], upd1(1), True, False),               # selectv t1 | select t2; t1 written
            ("t5_04", ["t2"], upd1(1), False, False),              # select t1 | selectv t2; t1 written
            ("t5_05", ["t1"], T2_KEYLESS_UPD, False, True),        # selectv t1 | select t2; t2 written
            ("t5_07", ["t1", "t2"], upd1(1), True, False),         # both arms selectv; t1 written
            ("t5_08", ["t1", "t2"], T2_KEYLESS_UPD, True, True)):  # both arms selectv; keyless t2 written
        txns, ev = union([locked(t) for t in arms], other, restore)
        out[f"range.{case}"] = dict(txns=txns, events=ev, commits=["T1"], expect_fail=["T1"] if fails else [],
                                    variants={"as_read": {}},
                                    reference_file=f"selectv_range.test/{case}.req")

    # recom t5_01: rows 1 and 2 inserted; T2 then T1 each count (plain) and
    # selectv `id < 10` (every row qualifies), then each moves every row's id
    # up by 2 (the update's own cursor captures nothing).  T2 commits first
    # and passes; T1 then finds T2's keys.
    moves = mov1(1, 3) + mov1(2, 4)
    out["recom.t5_01"] = dict(
        txns={"A1": auto(ins1(1)), "A2": auto(ins1(2)),
              "T2": sv([locked("t1")], moves), "T1": sv([locked("t1")], moves)},
        events=seq(("auto", "A1"), ("auto", "A2"), ("begin", "T2"), ("read", "T2"), ("begin", "T1"),
                   ("read", "T1"), ("commit", "T2"), ("commit", "T1")),
        commits=["T2", "T1"], expect_fail=["T1"],
        variants={"ran_off_end": {},
                  "bound": {t: [rng_("t1", 0, None, k(10), lflag=1)] for t in ("T1", "T2")}},
        reference_file="selectv_recom_range.test/t5_01.req")

    # recom t6_01: rows 2, 5, 9.  T1 counts `id > 3 and id < 7` and session 1
    # moves 5 -> 4 (into the range); T2 looks up id 4 and session 1 moves
    # 4 -> 5 (deleting the key read); T3 filters on id % 2 (no index serves
    # it: lock) and session 1 updates row 2's id to 2.  All fail.
    out["recom.t6_01"] = dict(
        txns={"A1": auto(ins1(2)), "A2": auto(ins1(5)), "A3": auto(ins1(9)),
              "T1": sv([rng_("t1", 0, k(3), k(9))]), "B1": auto(mov1(5, 4)),
              "T2": sv([point(4)]), "B2": auto(mov1(4, 5)),
              "T3": sv([locked("t1")]), "B3": auto(upd1(2))},
        events=seq(("auto", "A1"), ("auto", "A2"), ("auto", "A3"),
                   ("begin", "T1"), ("read", "T1"), ("auto", "B1"), ("commit", "T1"),
                   ("begin", "T2"), ("read", "T2"), ("auto", "B2"), ("commit", "T2"),
                   ("begin", "T3"), ("read", "T3"), ("auto", "B3"), ("commit", "T3")),
        commits=["T1", "T2", "T3"], expect_fail=["T1", "T2", "T3"],
        variants={"stop_row": {}, "bound": {"T1": [rng_("t1", 0, k(3), k(7))]}},
        reference_file="selectv_recom_range.test/t6_01.req")
    return out


def walk(req):
    """-> per commit statement of `req`, in order, 1 if its output holds the
    failure line.  A stepper file (every line starts with a session number)
    prints each statement's rows and then a line `done`; a plain file (one
    session through the SQL client) prints nothing for a commit that passes."""
    stmts = [l.strip() for l in open(req) if l.strip()]
    lines = [l.rstrip("\n") for l in open(req + ".out")]
    if all(re.match(r"\d+\s", s) for s in stmts):
        blocks, cur = [], []
        for l in lines:
            if l.strip() == "done":
                blocks.append(cur)
                cur = []
            else:
                cur.append(l)
        assert not cur and len(blocks) == len(stmts), (req, len(blocks), len(stmts))
        return [int(any(FAILED.search(l) for l in b)) for s, b in zip(stmts, blocks)
                if re.match(r"\d+\s+commit\b", s)]
    assert not any(re.search(r"failed|rc -?\d", l) for l in lines), req
    return [0 for s in stmts if re.match(r"commit\b", s)]


def main():
    from comdb2_amd.workloads import replay
    from helpers import commit_verdicts, model_check, selectv_cases, selectv_events
    sc = scenarios()
    total = failing = 0
    for name, s in sorted(sc.items()):
        s["reference_commits"] = walk(os.path.join(REF, s["reference_file"]))
        s["reference_file"] = "tests/" + s["reference_file"] + ".out"
        assert s["reference_commits"] == [int(n in s["expect_fail"]) for n in s["commits"]], \
            (name, s["reference_commits"], s["expect_fail"])
        total += len(s["reference_commits"])
        failing += sum(s["reference_commits"])
    assert (total, failing) == (20, 10), (total, failing)
    with open(os.path.join(HERE, "selectv_range.json"), "w") as f:
        json.dump(sc, f, indent=1, sort_keys=True)
    # the model on what the tests will read: every variant gives the
    # reference's verdicts, wherever between begin and the last read the
    # snapshot is taken
    check = lambda log, rs: model_check(log, rs)[0]
    for name, vname, v in selectv_cases():
        for snapshot in ("begin", "last_read"):
            got = commit_verdicts(v, replay(selectv_events(v, snapshot), check))
            assert got == v["reference_commits"], (name, vname, snapshot, got)
    print("wrote", len(sc), "scenarios,", total, "commits,", failing, "failing")


if __name__ == "__main__":
    main()
