"""Every probe path the dispatch (comdb2_amd/csrc/hsc_probe_host.cpp) can take,
through the public Validator API: the direct probe, the narrow tiles (bucket
table and 16-ary directory), the tile pipeline over narrow codes, the wide
pipeline, the compact tiles and the wide pipeline over compact codes.  Each
path answers (a) a plain batch, (b) a batch of table locks only -- nothing to
join, so the bucketed paths end in their flags tail -- and (c) the plain batch
after a few appended commits, which the delta probe answers beside the window
(and which decide whether a pack pass follows).  Each of them runs with the
timing off, on and off again: the verdicts equal the oracle's every time, and
with the timing on the six times are sane, `tiles` is the tile count of the
view the path joins over (0 on the direct probe) and `records` is what the
commit before the dispatch moved into its own file returned for the same call.
The small-batch path is off (PATH_NO_SMALL): every check reaches the dispatch.
A batch is synchronised before the next one, so what the narrow-tile kernels
store into the hot word is seen by the next batch's choice of path."""
import math

import numpy as np
import pytest

from comdb2_amd import formats as F
from comdb2_amd.formats import Range, ReadSets
from comdb2_amd.hsc import (LAYOUT_AUTO, LAYOUT_COMPACT, LAYOUT_COMPACT_WIDE, LAYOUT_NARROW,
                            LAYOUT_NARROW_CODES, LAYOUT_NARROW_DIRECT, LAYOUT_NARROW_TILES, LAYOUT_WIDE,
                            PATH_NO_SMALL, PATH_TILE_DIR, Validator)
from comdb2_amd.workloads import config2, config3
from test_incremental import log_slice

pytestmark = pytest.mark.gpu

TAIL_COMMITS = 30  # commits of situation (c) that arrive as appended writes
TIMES = ("locate_ms", "plan_ms", "scatter_ms", "join_ms", "pack_ms", "probe_total_ms")

# path -> (workload, layout set, build knob, layout reported, rows per tile of the view joined over)
PATHS = {
    "direct": ("c2", LAYOUT_NARROW_DIRECT, 0, LAYOUT_NARROW, None),
    "ntiles": ("c2", LAYOUT_NARROW_TILES, 0, LAYOUT_NARROW, 4096),
    "ntiles_dir": ("c2", LAYOUT_NARROW_TILES, PATH_TILE_DIR, LAYOUT_NARROW, 4096),
    "ncodes": ("c2", LAYOUT_NARROW_CODES, 0, LAYOUT_NARROW, 4096),
    "wide": ("c2", LAYOUT_WIDE, 0, LAYOUT_WIDE, 2048),
    "ctiles": ("c3", LAYOUT_AUTO, 0, LAYOUT_COMPACT, 2048),
    "cwide": ("c3", LAYOUT_COMPACT_WIDE, 0, LAYOUT_COMPACT, 2048),
}

# `records` of the timed batch of (path, situation), recorded by running this
# file on the commit before the probe dispatch left hsc_host.cpp (9f00618).
# (The counts are read from the path's scratch: a lock-only batch, which
# locates no record, reports what the batch before it left there.  None: not
# defined -- the compact window's lock-only batch takes the wide pipeline, whose
# count is the plan's bucket_off[ntiles], and no batch of the context has run
# that plan yet: the word is whatever the allocation held.)
RECORDS = {
    ("direct", "plain"): 0, ("direct", "locks"): 0, ("direct", "appended"): 0,
    ("ntiles", "plain"): 7688, ("ntiles", "locks"): 7688, ("ntiles", "appended"): 7610,
    ("ntiles_dir", "plain"): 8160, ("ntiles_dir", "locks"): 8160, ("ntiles_dir", "appended"): 8161,
    ("ncodes", "plain"): 7701, ("ncodes", "locks"): 0, ("ncodes", "appended"): 7723,
    ("wide", "plain"): 7858, ("wide", "locks"): 7858, ("wide", "appended"): 7885,
    ("ctiles", "plain"): 5493, ("ctiles", "locks"): None, ("ctiles", "appended"): 5497,
    ("cwide", "plain"): 11943, ("cwide", "locks"): 11943, ("cwide", "appended"): 11950,
}


def tail_writes(log, cut):
    """Records [cut, nrec) of log (whole commits) as append_writes rows."""
    rows, pend = [], []
    for i in range(cut, log.nrec):
        rt = int(log.rectype[i])
        if rt == F.REC_TXN_REGOP:
            rows += [(tb, ix, key, int(log.lsn[i])) for tb, ix, key in pend]
            pend = []
        elif int(log.table[i]) >= 0:
            tb = log.tbnames[int(log.table[i])]
            if rt in F.DTA_TYPES:
                pend.append((tb, -2, None))
            else:
                o = int(log.key_off[i])
                pend.append((tb, int(log.ix[i]), bytes(log.keys[o:o + int(log.keylen[i])])))
    assert not pend
    return rows


class Case:
    """A workload's log and read sets, its lock-only batch, the cut before its
    last TAIL_COMMITS commits, and the oracle's verdicts (computed once)."""

    def __init__(self, oracle_mod, log, rs):
        self.log, self.rs = log, rs
        regops = np.flatnonzero(log.rectype == F.REC_TXN_REGOP)
        self.cut = int(regops[-TAIL_COMMITS - 1]) + 1
        self.head = log_slice(log, 0, self.cut)
        self.tail = tail_writes(log, self.cut)
        self.rs_head = rs.with_snaps(np.minimum(rs.snap, self.head.lsn[-1]))
        # locks of every table at 64 of the batch's snapshots, and at the log's end
        snaps = [int(s) for s in rs.snap[:64]] + [int(log.end_lsn)] * 8
        self.locks = ReadSets.from_lists(
            [[Range.locked(log.tbnames[i % len(log.tbnames)])] for i in range(len(snaps))], snaps,
            tbnames=log.tbnames)
        check = lambda l, r: oracle_mod.check(l, r, nthreads=8)[0] != 0
        self.want = check(log, rs)
        self.want_head = check(self.head, self.rs_head)
        self.want_locks = check(log, self.locks)
        # both verdicts occur, among the locks too, and the appended commits decide some
        assert self.want.any() and not self.want.all()
        assert self.want_locks.any() and not self.want_locks.all()
        assert (self.want != self.want_head).any()


@pytest.fixture(scope="module")
def cases(oracle_mod):
    c2 = config2(n_commits=3000, n_txn=800, value_bits=20, width=1 << 10, snap_recent=0.5)
    return {"c2": Case(oracle_mod, c2.log, c2.readsets),
            "c3": Case(oracle_mod, *config3(n_writes=40000, n_txn=2000))}


def off_on_off(v, rs, want, what):
    """rs checked with the timing off, on, off: verdicts equal want each time.
    -> the timed run's timing."""
    timing = None
    for on in (False, True, False):
        v.enable_timing(on)
        got = v.check_readsets(rs) != 0
        v.synchronize()
        np.testing.assert_array_equal(got, want, err_msg=f"{what}, timing {on}")
        if on:
            timing = v.timing()
    return timing


def run_path(case, path):
    """-> {situation: (timing of the timed batch, the window's keys)}"""
    _, layout, knob, reported, _ = PATHS[path]
    out = {}
    v = Validator(0)
    try:
        v.set_paths(PATH_NO_SMALL | knob)
        v.set_layout(layout)
        v.ingest_log(case.log)
        out["plain"] = (off_on_off(v, case.rs, case.want, f"{path} plain"), v.keys)
        assert v.layout == reported
        out["locks"] = (off_on_off(v, case.locks, case.want_locks, f"{path} locks"), v.keys)
        v.ingest_log(case.head)
        np.testing.assert_array_equal(v.check_readsets(case.rs_head) != 0, case.want_head)
        v.synchronize()  # built: the tail goes to the delta run
        v.append_writes(case.tail, end_lsn=int(case.log.end_lsn))
        assert v.delta_rows > 0
        out["appended"] = (off_on_off(v, case.rs, case.want, f"{path} appended"), v.keys)
        assert v.delta_rows > 0 and v.layout == reported
    finally:
        v.close()
    return out


def expected_tiles(path, situation, keys):
    """Tiles of the view the batch joins over: none on the direct probe, which
    also answers a lock-only batch of a layout that is not forced to tiles."""
    rows = PATHS[path][4]
    if rows is None or (path == "ncodes" and situation == "locks"):
        return 0
    return -(-keys // rows)


@pytest.mark.parametrize("path", list(PATHS))
def test_probe_path(cases, path):
    out = run_path(cases[PATHS[path][0]], path)
    for situation, (t, keys) in out.items():
        print(f"{path} {situation}: keys {keys} tiles {t['tiles']} records {t['records']} "
              + " ".join(f"{k} {t[k]:.4f}" for k in TIMES))
    for situation, (t, keys) in out.items():
        what = f"{path} {situation}"
        legs = [t[k] for k in TIMES[:5]]
        assert all(math.isfinite(t[k]) and t[k] >= 0 for k in TIMES), (what, t)
        assert t["probe_total_ms"] >= max(legs), (what, t)
        assert t["tiles"] == expected_tiles(path, situation, keys), (what, t, keys)
        if RECORDS[(path, situation)] is not None:
            assert t["records"] == RECORDS[(path, situation)], (what, t)
