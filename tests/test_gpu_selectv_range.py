"""GPU: the reference's selectv range known answers
(tests/golden/selectv_range.json: tests/selectv_range.test and
tests/selectv_recom_range.test, restated) through every path a probe can take.

(a) Every entry, plain: each scenario and variant replayed commit by commit,
    the ordered verdicts equal to reference_commits, through check_readsets
    with the small path on and with PATH_NO_SMALL, through the drop-in
    bdb_osql_serial_check on a CurRangeArr with the window kept up to date by
    appends (both append modes: the other session's write arrives as a delta
    run or pending tail beside a built window), through the read set coalesced
    on the device, and through the commit-protocol harness, whose read-only
    selectv txns get their one full check.
(b) Every probe path of test_gpu_probe_paths.PATHS, with each scenario
    embedded in filler (tests/selectv_matrix.py): the scenario's first window
    row at offset 0, T - 1 and T of the path's tile size T, the checked read
    set first, last and at index 63 / 64 of batches of 1, 63, 64, 65 and 129
    read sets whose other verdicts are known by construction.  Every verdict
    of every batch is asserted against the reference / the construction and
    against the oracle on the same log.
(c) A two-member multi-GPU context on one GPU: pieces with the splitter right
    behind t1's keys and inside them, and replicas."""
import numpy as np
import pytest

import selectv_matrix as M
from comdb2_amd import formats as F
from comdb2_amd import hsc
from comdb2_amd.hsc import PATH_NO_SMALL, MultiValidator, Validator
from comdb2_amd.workloads import replay, replay_incremental
from helpers import commit_verdicts, selectv_cases, selectv_events
from test_gpu_probe_paths import PATHS

pytestmark = pytest.mark.gpu

CASES = selectv_cases()
SNAPSHOTS = ("begin", "last_read")
# Paths of PATHS that refuse these key shapes: {path: the refusing call's error}.
# None does: the narrow paths run on one-field filler keys, the compact ones on
# two-field filler keys that no 62-bit code holds (selectv_matrix.filler_key).
SKIPPED = {}
# path -> the filler keys that give the path's workload its layout
FILLER = {"c2": "narrow", "c3": "wide"}


def ingest_checker(v, coalesce=False):
    def check(log, rs):
        v.ingest_log(log)
        return v.check_readsets(v.coalesce(rs) if coalesce else rs)
    return check


def all_cases(run):
    """run(scenario, snapshot) -> {txn: rc} for every scenario, variant and
    snapshot; the ordered verdicts must be the reference's.  -> replays run"""
    n = 0
    for name, vname, sc in CASES:
        for snapshot in SNAPSHOTS:
            rcs = run(sc, snapshot)
            assert commit_verdicts(sc, rcs) == sc["reference_commits"], (name, vname, snapshot, rcs)
            n += 1
    return n


@pytest.fixture(scope="module")
def no_small():
    v = Validator(0)
    v.set_paths(PATH_NO_SMALL)
    yield v
    v.close()


def test_check_readsets_small_path_on(validator):
    all_cases(lambda sc, snapshot: replay(selectv_events(sc, snapshot), ingest_checker(validator)))


def test_check_readsets_no_small_path(no_small):
    all_cases(lambda sc, snapshot: replay(selectv_events(sc, snapshot), ingest_checker(no_small)))


@pytest.mark.parametrize("small", [True, False], ids=["small", "no_small"])
@pytest.mark.parametrize("mode", ["log", "writes"])
def test_drop_in_entry_on_an_appended_window(validator, no_small, mode, small):
    v = validator if small else no_small
    all_cases(lambda sc, snapshot: replay_incremental(selectv_events(sc, snapshot), v, mode=mode))


@pytest.mark.parametrize("small", [True, False], ids=["small", "no_small"])
def test_read_sets_coalesced_on_the_device(validator, no_small, small):
    v = validator if small else no_small
    all_cases(lambda sc, snapshot: replay(selectv_events(sc, snapshot), ingest_checker(v, coalesce=True)))


def test_commit_protocol_harness_checks_read_only_selectv(no_small):
    """hsc_harness_commit_protocol, one thread: a read-only selectv txn is
    checked (one full check, nothing logged), any other read-only txn is not."""
    v = no_small
    for name, vname, sc in CASES:
        events = selectv_events(sc)
        txns = [t for e, t in events if e == "begin"]
        v.ingest_log(F.LogBuilder().build())
        rc, seq, snap, cend, st = v.commit_protocol(txns, events, 1)
        got = {t.name: int(rc[i]) for i, t in enumerate(txns)}
        assert commit_verdicts(sc, got) == sc["reference_commits"], (name, vname, got)
        for i, t in enumerate(txns):
            if not t.writes:
                assert seq[i] == -1, (name, t.name)                       # logs nothing
                assert (cend[i] != 0) == bool(t.selectv and t.reads), (name, t.name)  # checked or not
            else:
                assert (seq[i] >= 0) == (rc[i] == 0), (name, t.name)


# --------------------------------------------------------------------------- (b)
@pytest.fixture(scope="module")
def windows(oracle_mod):
    """{(T, filler kind): [Window]}, built once per shape; the oracle's verdicts
    on each window's pool are a third witness, and must be the constructed ones
    -- a disagreement here is a failure of the oracle, not of a probe path."""
    cache = {}

    def get(T, kind):
        if (T, kind) not in cache:
            ws = M.build(T, kind)
            for w in ws:
                w.oracle = oracle_mod.check(w.log, w.pool, nthreads=8)[0] != 0
                np.testing.assert_array_equal(
                    w.oracle, w.want, err_msg=f"the ORACLE disagrees with the reference value: {w.what}")
            cache[(T, kind)] = ws
        return cache[(T, kind)]
    return get


def first_row_of_t1(v, gids):
    """-> (rows in front of t1's first row, t1's rows) of the built window"""
    gid, _, _ = v.export_window()
    return int((gid < gids[1]).sum()), int((gid == gids[1]).sum())


@pytest.mark.parametrize("path", list(PATHS))
def test_probe_path_matrix(windows, path):
    if path in SKIPPED:
        pytest.skip(SKIPPED[path])
    workload, layout, knob, reported, rows = PATHS[path]
    T = rows or 4096            # the direct probe has no tiles: the narrow tiles' size
    kind = FILLER[workload]
    ws = windows(T, kind)
    ran, seen_offsets = 0, set()
    v = Validator(0)
    try:
        v.set_paths(PATH_NO_SMALL | knob)
        v.set_layout(layout)
        gids = M.register_groups(v, kind)
        for w in ws:
            v.ingest_log(w.log)
            for (n, p), idx in w.batches():
                timed = (n, p) == (M.POOL, M.POOL - 1)
                v.enable_timing(timed)
                got = v.check_readsets(w.pool.subset(idx)) != 0
                v.synchronize()
                if timed:
                    # a batch dense enough for the path's tiles joined over all of them (the
                    # direct probe over none): the path under test answered, not another one
                    tiles = v.timing()["tiles"]
                    assert tiles == (0 if rows is None else -(-v.keys // rows)), (path, w.what, tiles, v.keys)
                what = f"{path}: {w.what}, batch of {n}, read set at {p}"
                assert bool(got[p]) == bool(w.want[0]), f"{what}: not the reference's verdict"
                np.testing.assert_array_equal(got, w.want[idx], err_msg=f"{what}: a decoy's verdict")
                np.testing.assert_array_equal(got, w.oracle[idx], err_msg=f"{what}: not the oracle's")
                ran += 1
            assert v.layout == reported, (path, w.what, v.layout)
            offset = int(w.what.split(" offset ")[1].split()[0])
            if "recom.t6_01-stop_row" in w.what and w.what.endswith("commit T1"):
                # by construction, once per offset: t1's four rows (ids 2, 5, 9 and the 4 that
                # 5 moved to) start at row `offset` of the window, and at T - 1 they straddle
                # the tile boundary
                front, mine = first_row_of_t1(v, gids)
                assert (front, mine) == (offset, 4), (w.what, front, mine)
                assert v.keys > T                                   # more than one tile
                seen_offsets.add(offset)
    finally:
        v.close()
    assert seen_offsets == {0, T - 1, T}
    print(f"{path}: T {T}, {kind} filler, {len(ws)} windows, {ran} (scenario, variant, commit, offset, batch) "
          "combinations")
    assert ran == len(ws) * 12 and len(ws) == 3 * 24


# --------------------------------------------------------------------------- (c)
def key_word(k):
    """A key of at most 8 bytes as the window's first big-endian word."""
    return int.from_bytes(k.ljust(8, b"\0"), "big")


def t1_key(i):
    return bytes([0x08]) + ((i ^ (1 << 31)) & 0xFFFFFFFF).to_bytes(4, "big")


@pytest.mark.parametrize("placement", ["pieces_behind_t1", "pieces_inside_t1", "replicas"])
def test_two_member_context(placement):
    """Pieces: the splitter right behind every t1 key (member 1's piece starts
    where a table after t1 would; the keyless t2 has no rows anywhere, only
    table maxima, so range.t5_08's lock on t2 is answered on member 0 from a
    data record alone), or inside t1 at id 3 (recom.t6_01's range and
    recom.t5_01's bound lie on or across it).  Replicas: every member holds
    the window.  Through check_readsets on the ingested log and through the
    drop-in entry on a window kept up to date by appended log records, which
    are routed to their owners."""
    m = MultiValidator([0, 0])
    try:
        m.set_mode(hsc.MULTI_REPLICAS if placement == "replicas" else hsc.MULTI_PIECES)
        g = m.register_group("t1", 0, 5)
        if placement == "pieces_behind_t1":
            m.set_splitters(np.array([g + 1], np.uint32), np.array([[0]], np.uint64))
        elif placement == "pieces_inside_t1":
            m.set_splitters(np.array([g], np.uint32), np.array([[key_word(t1_key(3))]], np.uint64))
        all_cases(lambda sc, snapshot: replay(selectv_events(sc, snapshot), ingest_checker(m)))
        assert m.mode == (hsc.MULTI_REPLICAS if placement == "replicas" else hsc.MULTI_PIECES)
        all_cases(lambda sc, snapshot: replay_incremental(selectv_events(sc, snapshot), m, mode="log"))
    finally:
        m.close()
