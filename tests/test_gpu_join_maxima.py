"""GPU parity of the narrow join's range-maximum step (wave_any_after32,
comdb2_amd/csrc/hsc_device.h): a wave's records whose ranges the two-read
filter cannot decide are resolved four per pass by 16-lane groups.

Every case is one index of int64 keys on the 8-byte-row tile pipeline
(LAYOUT_NARROW_TILES), verdicts bit for bit against the oracle.  The window is
3,000 commits x 6 keys over 2^20 values: about 17.8k distinct rows, four full
4096-row tiles and a partial fifth, about 59 values per row."""

import numpy as np
import pytest

from comdb2_amd import formats as F
from comdb2_amd.formats import LogBuilder, Range, ReadSets
from comdb2_amd.hsc import LAYOUT_AUTO, LAYOUT_NARROW, LAYOUT_NARROW_TILES

pytestmark = pytest.mark.gpu

VALUES = 1 << 20
PER_ROW = 58   # values per distinct row, rounded down
TILE = 4096    # rows per tile (kTLog2)
TILE_CAP = 1024  # records a tile's own block takes (kTileCap); the rest are overflow items


def keyed_case(seed, range_fn, n_txn, snap_recent=0.3, snap_at=None, n_commits=3000, per_commit=6,
               ranges_per_txn=8):
    """keyed_case of test_gpu_narrow.py on the window above, returning also
    the sorted distinct keys and the ranges' bounds (for row counts in numpy).
    snap_at = "before": every snapshot older than every commit, "end": every
    snapshot at the log's end; else among the most recent snap_recent."""
    rng = np.random.default_rng(seed)
    lb = LogBuilder(step=64)
    commits = [lb.next_lsn()]
    keys = []
    for c in range(n_commits):
        lb.begin(c)
        for _ in range(per_commit):
            k = int(rng.integers(0, VALUES))
            keys.append(k)
            lb.write(c, F.REC_UNDO_UPD_IX, "t1", 0, F.enc_int64(k))
        commits.append(lb.commit(c))
    log = lb.build()
    recent = max(1, int(len(commits) * snap_recent))
    sets, snaps, bounds = [], [], []
    for _ in range(n_txn):
        rs = []
        for _ in range(ranges_per_txn):
            a, b = range_fn(rng)
            bounds.append((a, b))
            rs.append(Range("t1", 0, F.enc_int64(a), F.enc_int64(b)))
        sets.append(rs)
        if snap_at == "before":
            snaps.append(commits[0])
        elif snap_at == "end":
            snaps.append(commits[-1])
        else:
            snaps.append(commits[len(commits) - 1 - int(rng.integers(0, recent))])
    rows = np.unique(np.asarray(keys, dtype=np.int64))
    bounds = np.asarray(bounds, dtype=np.int64)
    pa = np.searchsorted(rows, bounds[:, 0], side="left")
    pb = np.searchsorted(rows, bounds[:, 1], side="right")
    return log, ReadSets.from_lists(sets, snaps, tbnames=lb.tbnames), rows, pa, pb


def mixed_widths(rng):
    """80 % of the ranges below 48 rows, 15 % below 700, 5 % anywhere."""
    a = int(rng.integers(0, VALUES))
    u = rng.random()
    if u < 0.80:
        w = int(rng.integers(0, PER_ROW * 48))
    elif u < 0.95:
        w = int(rng.integers(0, PER_ROW * 700))
    else:
        w = int(rng.integers(0, VALUES))
    return a, a + w


def tile_records(pa, pb):
    """Join records per tile: a non-empty range leaves one in the tile of its
    first row and one in the tile of its last row where that is another."""
    ne = pa < pb
    ta, tb = pa[ne] // TILE, (pb[ne] - 1) // TILE
    nt = int(tb.max()) + 1
    return np.bincount(ta, minlength=nt) + np.bincount(tb[tb != ta], minlength=nt)


def run_tiles(v, oracle_mod, log, rs):
    want, _, _ = oracle_mod.check(log, rs, nthreads=8)
    try:
        v.set_layout(LAYOUT_NARROW_TILES)
        v.ingest_log(log)
        assert v.layout == LAYOUT_NARROW
        got = v.check_readsets(rs)
    finally:
        v.set_layout(LAYOUT_AUTO)
    np.testing.assert_array_equal(got != 0, want != 0)
    return want != 0


@pytest.mark.parametrize("snap_recent", [0.02, 1.0])
def test_range_lengths_and_block_boundaries(validator, oracle_mod, snap_recent):
    """Every row count from 1 to 40 at every offset inside the 16- and
    128-row blocks, long ranges through the b16 / b128 slots; at 0.02 a block
    maximum often beats r(S) where no row of the range does, at 1.0 a row
    often does.  Every full tile is above kTileCap, so the overflow items'
    blocks run too."""
    log, rs, rows, pa, pb = keyed_case(31, mixed_widths, 900, snap_recent=snap_recent)
    assert 4 * TILE < len(rows) < 5 * TILE
    cnt = pb - pa
    seen = np.bincount(cnt[cnt <= 40], minlength=41)
    assert (seen[1:41] > 0).all()
    assert int((cnt > 16).sum()) >= 100
    assert int((cnt >= 128).sum()) >= 100
    assert (tile_records(pa, pb)[:4] > TILE_CAP).all()
    bad = run_tiles(validator, oracle_mod, log, rs)
    assert bad.any() and not bad.all()


@pytest.mark.parametrize("snap_recent", [0.02, 1.0])
def test_one_range_per_read_set(validator, oracle_mod, snap_recent):
    """The same ranges one per read set, so that every range's own verdict is
    compared (among eight, one range's hit hides another's miss)."""
    log, rs, rows, pa, pb = keyed_case(35, mixed_widths, 7200, snap_recent=snap_recent,
                                       ranges_per_txn=1)
    assert (tile_records(pa, pb)[:4] > TILE_CAP).all()
    bad = run_tiles(validator, oracle_mod, log, rs)
    assert 0.05 < bad.mean() < 0.95


def test_few_records_per_tile(validator, oracle_mod):
    """About 70 records per tile: the last wave with records is partial, the
    later waves and the second round have none."""
    log, rs, rows, pa, pb = keyed_case(32, mixed_widths, 40, snap_recent=0.05)
    per_tile = tile_records(pa, pb)
    assert per_tile.max() < 512 and (per_tile % 64 != 0).any()
    bad = run_tiles(validator, oracle_mod, log, rs)
    assert bad.any() and not bad.all()


@pytest.mark.parametrize("snap_at", ["before", "end"])
def test_all_lanes_pending_or_none(validator, oracle_mod, snap_at):
    """Snapshots older than every commit: every non-empty range is a hit (all
    of a wave's lanes pending); snapshots at the log's end: none is."""
    log, rs, rows, pa, pb = keyed_case(33, mixed_widths, 300, snap_at=snap_at)
    bad = run_tiles(validator, oracle_mod, log, rs)
    if snap_at == "before":
        nonempty = (pa < pb).reshape(300, 8).any(axis=1)
        assert nonempty.any()
        np.testing.assert_array_equal(bad, nonempty)
    else:
        assert not bad.any()


@pytest.mark.parametrize("snap_recent", [0.02, 1.0])
def test_partial_last_tile(validator, oracle_mod, snap_recent):
    """Ranges over the fifth tile's rows whose upper bound lies past the
    window's last key (tn < T), some of them wholly past it."""
    def top(rng):
        # the lower bound: 60 % within 40 rows of the end, 30 % within 1,500,
        # 10 % past it; the upper bound: 85 % past the last key
        u = rng.random()
        if u < 0.6:
            a = VALUES - int(rng.integers(0, PER_ROW * 40))
        elif u < 0.9:
            a = VALUES - int(rng.integers(0, PER_ROW * 1500))
        else:
            a = VALUES + int(rng.integers(0, PER_ROW * 8))
        if rng.random() < 0.85:
            return a, VALUES + int(rng.integers(PER_ROW * 8, 1 << 12))
        return a, a + int(rng.integers(0, PER_ROW * 48))
    # (two ranges per read set: most ranges here reach the newest rows, and a
    # read set is clean only if all of its ranges are)
    log, rs, rows, pa, pb = keyed_case(34, top, 1200, snap_recent=snap_recent, ranges_per_txn=2)
    last = len(rows)
    assert last % TILE != 0
    assert int(((pb == last) & (pa < pb)).sum()) >= 100      # clipped at the last row
    assert int(((pb == last) & (pa // TILE == last // TILE) & (pa < pb)).sum()) >= 100
    assert int((pa == last).sum()) > 0                       # wholly past the last key
    bad = run_tiles(validator, oracle_mod, log, rs)
    assert bad.any() and not bad.all()
