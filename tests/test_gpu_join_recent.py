"""GPU parity of the narrow join's recent lists (k_recent and join_s_item,
comdb2_amd/csrc/hsc_narrow.hip): a join block stages its tile's 256 newest
rows and walks its records over them; a round with a live record whose
snapshot is older than a row left out (r(S) < rtheta[t]) stages the whole tile
instead and counts itself in hsc_batch_stats.full_tile_joins.

Windows are built as in test_gpu_join_column.py: one index of distinct int64
keys KEY0 + KEY_STEP i ingested as device rows (LAYOUT_NARROW_TILES), three
full 4096-row tiles and a partial one unless a case says otherwise, commit
LSNs spanning < 2^32.  Every batch is probed with hsc_probe_device into
verdict bytes prefilled with 0xFF and compared bit for bit with the CPU
sort-join (oracle/sortjoin.c).  The lists, their members and rtheta come from
the numpy model (tests/recent_model.py) over the rows' LSNs: ranks grow with
the LSN in both rank modes, so r(S) >= rtheta[t] <=> S >= the model's theta.

A batch that must stay on the lists has every snapshot at or above the theta
of the tile it probes (asserted from the model), so the reference alone says
full_tile_joins may not move; a batch that must leave them has a snapshot one
below.  A range whose lower bound is a tile's first key also leaves a record
(one that meets no row) in the tile before, which that tile's block judges by
its own rtheta: the batches that count blocks keep off the tiles' first rows
or keep such snapshots above the neighbour's theta.  The log-mode window of test_modes needs 17 tiles for the build to
consider log buckets at all; it has 20.
"""

import numpy as np
import pytest

import appended_model as A
import recent_model as M
from comdb2_amd import hsc
from comdb2_amd.hsc import LAYOUT_NARROW, LAYOUT_NARROW_TILES, PATH_NO_SMALL, Validator
from comdb2_amd.workloads import int64_words
from test_gpu_appended_placed import append
from test_gpu_join_column import launch, outputs, paths, probe, result, upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE, R = M.TILE, M.R
CHUNK, TILE_CAP = 4096, 1024
KEY0, KEY_STEP = 1000, 7
LSN0 = (5 << 32) + 4096
PARTIAL = 777


class Win:
    """Rows in key order (one group), their lists by the model and the
    sort-join over them.  words: 2 = 9-byte int64 keys, 1 = 8-byte keys."""

    def __init__(self, keys, lsn, words=2):
        self.keys = np.asarray(keys, np.int64)
        self.lsn = np.asarray(lsn, np.uint64)
        assert len(self.keys) == len(self.lsn) and (np.diff(self.keys) > 0).all()
        self.nwords = words
        self.klen = 9 if words == 2 else 8
        self.words = self.enc(self.keys)
        self.ntiles = (len(self.keys) + TILE - 1) // TILE
        self.lists = M.window_lists(self.lsn)
        self.theta = np.array([th for _, th in self.lists], np.uint64)
        self.sj = None

    def enc(self, vals):
        vals = np.asarray(vals, np.int64)
        return int64_words(vals) if self.nwords == 2 else vals.astype(np.uint64).reshape(1, -1).copy()

    def tile_of(self, rows):
        return np.asarray(rows, np.int64) // TILE

    def out_rows(self, t, first=True):
        """Rows of tile t left out of its list (first=False: but for the tile's first row)."""
        a, b = t * TILE, min((t + 1) * TILE, len(self.keys))
        return np.setdiff1d(np.arange(a if first else a + 1, b), self.lists[t][0])

    def reference(self, oracle_mod, m, table_max):
        if self.sj is None:
            self.sj = oracle_mod.SortJoin(np.zeros(len(self.lsn), np.uint32), self.words, self.lsn, 1)
        want, _ = self.sj.probe(m, table_max, nthreads=8)
        return want != 0

    def close(self):
        if self.sj is not None:
            self.sj.close()
            self.sj = None


def distinct_lsns(n, seed, step=1):
    """Every row its own commit: LSN0 + step (1 + a permutation of the rows)."""
    return np.uint64(LSN0) + np.uint64(step) * (1 + np.random.default_rng(seed).permutation(n).astype(np.uint64))


def plain_keys(n):
    return KEY0 + KEY_STEP * np.arange(n, dtype=np.int64)


def make_batch(w, lo, hi, snap):
    """One range per read set, in batch order."""
    n = len(lo)
    z32 = np.zeros(0, np.uint32)
    return dict(words=w.nwords, n=n, n_lock=0, n_txn=n, lo=w.enc(lo), hi=w.enc(hi),
                lo_vals=np.asarray(lo, np.int64), hi_vals=np.asarray(hi, np.int64),
                gid=np.zeros(n, np.uint32), snap=np.asarray(snap, np.uint64),
                txn=np.arange(n, dtype=np.uint32), lock_table=z32, lock_snap=np.zeros(0, np.uint64),
                lock_txn=z32, forced=np.zeros(n, np.uint8))


def points(w, rows, snap):
    """A point range on each of `rows`."""
    return make_batch(w, w.keys[rows], w.keys[rows], snap)


def ranges(w, tiles, seed):
    """One range inside each tile of `tiles`: rows r0 .. r0 + k, k < 40, from
    the first row's key to the last one's.  Returns (lo, hi, newest LSN inside)."""
    rng = np.random.default_rng(seed)
    tiles = np.asarray(tiles, np.int64)
    rows = np.minimum(TILE, len(w.keys) - tiles * TILE)
    k = np.minimum(rng.integers(0, 40, len(tiles)), rows - 1)
    pa = tiles * TILE + rng.integers(0, 1 << 30, len(tiles)) % (rows - k)
    pb = pa + k + 1
    return w.keys[pa], w.keys[pb - 1], M.range_max(w.lsn.astype(np.int64), pa, pb).astype(np.uint64)


def recent_batch(w, n, seed):
    """n ranges over all tiles whose snapshots are the newest LSN inside the
    range or the one before, raised to the window's largest theta."""
    rng = np.random.default_rng(seed)
    tiles = np.arange(n) % w.ntiles
    lo, hi, newest = ranges(w, tiles, seed)
    snap = np.maximum(newest - rng.integers(0, 2, n).astype(np.uint64), w.theta.max())
    assert on_lists(w, w.tile_of(np.searchsorted(w.keys, lo)), snap)
    return make_batch(w, lo, hi, snap)


def old_batch(w, n, seed, tiles=None):
    """n point ranges on rows left out of their tile's list, snapshot = the LSN before the row's."""
    rng = np.random.default_rng(seed)
    tiles = [t for t in range(w.ntiles) if len(w.out_rows(t))] if tiles is None else tiles
    rows = np.concatenate([rng.choice(w.out_rows(t, first=False), -(-n // len(tiles))) for t in tiles])[:n]
    snap = w.lsn[rows] - np.uint64(1)
    assert (snap < w.theta[w.tile_of(rows)]).all()
    return make_batch(w, w.keys[rows], w.keys[rows], snap)


def cat(w, *ms):
    """The batches' ranges as one batch."""
    return make_batch(w, np.concatenate([m["lo_vals"] for m in ms]), np.concatenate([m["hi_vals"] for m in ms]),
                      np.concatenate([m["snap"] for m in ms]))


def on_lists(w, tiles, snap):
    """Every snapshot is at or above the theta of the tile its range lies in."""
    return bool((np.asarray(snap, np.uint64) >= w.theta[tiles]).all())


# ---- device side -----------------------------------------------------------
@pytest.fixture
def make_validator():
    made = []

    def make(w, fold=None, path_flags=0):
        v = Validator(0)
        made.append(v)
        assert v.register_group("t1", 0, w.klen) == 0
        v.set_layout(LAYOUT_NARROW_TILES)
        if path_flags:
            v.set_paths(path_flags)
        if fold:
            v.set_fold(*fold)
        dev = torch.device("cuda", 0)
        tg = torch.zeros(len(w.keys), dtype=torch.int32, device=dev)
        tw = torch.from_numpy(w.words.reshape(-1).view(np.int64)).to(dev)
        tl = torch.from_numpy(w.lsn.view(np.int64)).to(dev)
        v.ingest_device(len(w.keys), w.nwords, tg.data_ptr(), tw.data_ptr(), tl.data_ptr(), int(w.lsn.max()) + 1)
        torch.cuda.synchronize()
        assert v.layout == LAYOUT_NARROW
        return v

    yield make
    for v in made:
        v.close()


def full_joins(v):
    return v.batch_stats()["full_tile_joins"]


def check(v, w, oracle_mod, m, rise, bitmap=True, mixed=True):
    """Probe m: verdicts equal the sort-join's, full_tile_joins rises by
    `rise` (an int, or (least, most))."""
    want = w.reference(oracle_mod, m, v.table_max())
    if mixed:
        assert 0 < int(want.sum()) < len(want)
    before = full_joins(v)
    got = probe(v, m, bitmap)
    np.testing.assert_array_equal(got, want)
    lo, hi = (rise, rise) if isinstance(rise, int) else rise
    assert lo <= full_joins(v) - before <= hi
    return want


_wins = {}


def base_window():
    """Three full tiles and one of 777 rows, every row a commit of its own."""
    if "base" not in _wins:
        n = 3 * TILE + PARTIAL
        _wins["base"] = Win(plain_keys(n), distinct_lsns(n, 11))
    return _wins["base"]


@pytest.fixture(scope="module", autouse=True)
def _close_windows():
    yield
    for w in _wins.values():
        w.close()
    _wins.clear()


# ---- members and the cut ------------------------------------------------------
def test_members(make_validator, oracle_mod):
    """Every list member of every tile, probed alone: the LSN before its own
    as snapshot conflicts, its own does not; no block leaves its list."""
    w = base_window()
    v = make_validator(w)
    rows = np.concatenate([m for m, _ in w.lists])
    assert len(rows) == 4 * R
    both = np.concatenate([rows, rows])
    snap = np.concatenate([w.lsn[rows] - np.uint64(1), w.lsn[rows]])
    assert on_lists(w, w.tile_of(both), snap)
    want = check(v, w, oracle_mod, points(w, both, snap), 0)
    np.testing.assert_array_equal(want, np.arange(len(both)) < len(rows))
    assert paths(v) == (1, 0)


def test_cut(make_validator, oracle_mod):
    """The newest row left out of each tile (rank = rtheta) with the LSN before
    it as snapshot: found, by blocks that staged their tile.  A member with
    the snapshot at rtheta exactly: found on the list."""
    w = base_window()
    v = make_validator(w)
    cut = np.array([w.out_rows(t)[np.argmax(w.lsn[w.out_rows(t)])] for t in range(w.ntiles)])
    np.testing.assert_array_equal(w.lsn[cut], w.theta)
    want = check(v, w, oracle_mod, points(w, cut, w.lsn[cut] - np.uint64(1)), (1, w.ntiles), mixed=False)
    assert want.all()
    mem = np.array([m[0] for m, _ in w.lists])
    want = check(v, w, oracle_mod, points(w, mem, w.theta), 0, mixed=False)
    assert want.all()
    # ... and at rtheta the row at the cut itself is no conflict, still on the list
    want = check(v, w, oracle_mod, points(w, cut, w.theta), 0, mixed=False)
    assert not want.any()


def test_ties_at_the_cut(make_validator, oracle_mod):
    """10 rows per LSN (9 for the newest), so the cut of every full tile falls
    inside a commit's rows: the earlier ones are members, the later ones not."""
    n = 3 * TILE + PARTIAL
    rng = np.random.default_rng(5)
    commit = np.concatenate([(rng.permutation(min(TILE, n - a)) + 3) // 10 for a in range(0, n, TILE)])
    w = _wins["ties"] = Win(plain_keys(n), np.uint64(LSN0 + 1) + 2 * commit.astype(np.uint64))
    v = make_validator(w)
    tin, tout = [], []
    for t in range(3):
        m = w.lists[t][0]
        a, b = m[w.lsn[m] == w.theta[t]], w.out_rows(t)[w.lsn[w.out_rows(t)] == w.theta[t]]
        assert len(a) and len(b) and a.max() < b.min() and len(a) + len(b) == 10
        tin.append(a[a % TILE != 0]), tout.append(b[b % TILE != 0])
    tin, tout = np.concatenate(tin), np.concatenate(tout)
    for rows in (tin, tout):
        th = w.theta[w.tile_of(rows)]
        want = check(v, w, oracle_mod, points(w, rows, th - np.uint64(1)), (1, 3), mixed=False)
        assert want.all()
        want = check(v, w, oracle_mod, points(w, rows, th), 0, mixed=False)
        assert not want.any()
    # whole commits around the cut: ranges over the tile at both snapshots
    lo = np.array([w.keys[t * TILE] for t in range(3)])
    hi = np.array([w.keys[t * TILE + TILE - 2] for t in range(3)])
    check(v, w, oracle_mod, make_batch(w, np.tile(lo, 2), np.tile(hi, 2),
                                       np.concatenate([w.theta[:3], w.lsn.max() + np.zeros(3, np.uint64)])), 0)


@pytest.mark.parametrize("last", [1, 255, 256, 257])
def test_short_lists(make_validator, oracle_mod, last):
    """A last tile of `last` rows: up to 256 every row is a member (rtheta = 0,
    any snapshot takes the list), 257 leave one out."""
    n = TILE + last
    # (the full tile's rows are the older ones: no snapshot below is older than its theta)
    lsn = np.concatenate([distinct_lsns(TILE, last), distinct_lsns(last, last + 1) + np.uint64(TILE)])
    w = _wins[f"short{last}"] = Win(plain_keys(n), lsn)
    v = make_validator(w)
    assert w.theta[1] == (0 if last <= R else w.lsn[TILE:].min()) and w.theta[0] < w.lsn[TILE:].min()
    rows = np.arange(TILE, n)
    both = np.concatenate([rows, rows, rows])
    snap = np.concatenate([w.lsn[rows] - np.uint64(1), w.lsn[rows], np.full(last, w.theta[0], np.uint64)])
    keep = snap >= w.theta[1]
    want = check(v, w, oracle_mod, points(w, both[keep], snap[keep]), 0, mixed=False)
    assert want.any() and not want.all()
    # a range over the whole short tile and past the window's last key
    m = make_batch(w, [w.keys[TILE] - 1] * 2, [w.keys[-1] + 50] * 2, [w.lsn[rows].max(), max(w.lsn[rows].max() - np.uint64(1), w.theta[1])])
    check(v, w, oracle_mod, m, 0)
    if last > R:
        out = w.out_rows(1)
        assert len(out) == 1 and w.lsn[out[0]] == w.theta[1]
        want = check(v, w, oracle_mod, points(w, out, w.lsn[out] - np.uint64(1)), 1, mixed=False)
        assert want.all()


# ---- batches --------------------------------------------------------------------
@pytest.mark.parametrize("bitmap", [True, False], ids=["bitmap", "bytes"])
def test_mixed_batch(make_validator, oracle_mod, bitmap):
    """5,000 recent-snapshot ranges over all tiles and 20 old-snapshot ones in
    tile 1: that tile alone is staged whole, once per batch.  1255 records a
    tile: the first batch runs them in rounds on the column path, the next two
    take the plan path, where the old ones (the batch's last, past record 1024
    of their tile) fall to one overflow item."""
    w = base_window()
    v = make_validator(w)
    m = cat(w, recent_batch(w, 5000, 21), old_batch(w, 20, 22, tiles=[1]))
    for k in range(2):
        check(v, w, oracle_mod, m, 1, bitmap)
    check(v, w, oracle_mod, recent_batch(w, 5000, 23), 0, bitmap)
    assert paths(v) == (1, 2)


def test_hot_tile(make_validator, oracle_mod):
    """1524 records in tile 2, the only old-snapshot one among those of the
    second chunk -- records 1024 and up of the tile, its second round.  First
    on the column path (rounds inside the tile's block: the first stays on the
    list, the second stages the tile), then the same batch on the plan path
    (the tile's block takes records 0 .. 1023, an overflow item the rest)."""
    w = base_window()
    v = make_validator(w)
    other = np.array([0, 1, 3])
    tiles = np.concatenate([np.full(TILE_CAP, 2), other[np.arange(CHUNK - TILE_CAP) % 3],  # chunk 0
                            np.full(499, 2), other[np.arange(600) % 3]])                  # chunk 1
    lo, hi, newest = ranges(w, tiles, 31)
    rng = np.random.default_rng(32)
    snap = np.maximum(newest - rng.integers(0, 2, len(tiles)).astype(np.uint64), w.theta.max())
    m1 = make_batch(w, lo, hi, snap)
    m = cat(w, m1, old_batch(w, 1, 33, tiles=[2]))
    assert m["n"] > CHUNK and (np.bincount(tiles)[2] + 1) == 1524
    check(v, w, oracle_mod, m, 1)
    assert paths(v) == (1, 0)
    check(v, w, oracle_mod, m, 1)
    assert paths(v) == (1, 1)
    # nothing old: both paths stay on the lists (the batch after a hot one takes the plan)
    check(v, w, oracle_mod, m1, 0)
    assert paths(v) == (1, 2)


def skewed_window(ntiles=20, sparse=8):
    """Dense keys, then `sparse` tiles of keys 2^20 apart: the build takes the
    bucket table's log mode, and its batches the plan path."""
    n = (ntiles - 1) * TILE + PARTIAL
    nd = (ntiles - sparse) * TILE
    keys = np.concatenate([KEY0 + np.arange(nd, dtype=np.int64),
                           KEY0 + nd + (np.arange(1, n - nd + 1, dtype=np.int64) << 20)])
    return Win(keys, distinct_lsns(n, 41))


MODES = {
    "log-mode": (skewed_window, (0, 1)),
    # commits 2^21 apart span >= 2^32: ranks come from the commit directory
    "directory-ranks": (lambda: Win(plain_keys(3 * TILE + PARTIAL), distinct_lsns(3 * TILE + PARTIAL, 42, 1 << 21)), (1, 0)),
    "one-word-keys": (lambda: Win(plain_keys(3 * TILE + PARTIAL), distinct_lsns(3 * TILE + PARTIAL, 43), words=1), (1, 0)),
}


@pytest.mark.parametrize("mode", list(MODES))
def test_modes(make_validator, oracle_mod, mode):
    make, first_path = MODES[mode]
    w = _wins[mode] = make()
    if mode == "directory-ranks":
        assert int(w.lsn.max() - w.lsn.min()) >= 1 << 32
    v = make_validator(w)
    check(v, w, oracle_mod, recent_batch(w, 6000, 51), 0)
    assert paths(v) == first_path
    nout = sum(1 for t in range(w.ntiles) if len(w.out_rows(t)))
    check(v, w, oracle_mod, cat(w, recent_batch(w, 3000, 52), old_batch(w, 40 * nout, 53)), (nout, nout))
    check(v, w, oracle_mod, recent_batch(w, 6000, 54), 0)


# ---- rebuilds -------------------------------------------------------------------
@pytest.mark.parametrize("background", [False, True], ids=["inline", "background"])
def test_rebuild(make_validator, oracle_mod, background):
    """750 rows appended in three pieces, keys between the window's, each newer
    than every row before: a fold at 600 rows, inline or in the background.
    After every piece and after the last fold the appended rows are probed at
    their LSN and the one before, with recent ranges: the folded window's
    newest rows are the appended ones, so its lists must be new."""
    w = base_window()
    v = make_validator(w, fold=(600, background), path_flags=PATH_NO_SMALL)
    n = len(w.keys)
    rng = np.random.default_rng(61)
    at = np.sort(rng.choice(n - 1, 750, replace=False))
    order = rng.permutation(750)
    end = int(w.lsn.max()) + 1
    app = A.Rows(np.zeros(750, np.uint32), int64_words(w.keys[at] + 3), np.uint64(end) + order.astype(np.uint64))
    before = full_joins(v)
    done = np.zeros(750, bool)
    for piece in range(4):
        if piece < 3:
            sel = np.flatnonzero(order // 250 == piece)
            sel = sel[np.argsort(order[sel])]  # in commit order
            append(v, app.take(sel))
            done[sel] = True
            if not background and v.delta_rows >= 600:
                v.export_window()  # (hsc_probe_device takes no window with an inline fold due)
        else:
            v.export_window()  # folds whatever run is left
            assert v.delta_rows == 0
        u = union(w, at[done], app.lsn[done])
        rows = np.flatnonzero(u.lsn >= end)
        both = np.concatenate([rows, rows])
        snap = np.concatenate([u.lsn[rows] - np.uint64(1), u.lsn[rows]])
        floor = max(int(w.theta.max()), int(u.theta.max()))  # main window or folded: on the lists
        rb = recent_batch(u, 3000, 62 + piece)
        rb["snap"] = np.maximum(rb["snap"], np.uint64(floor))
        m = cat(u, points(u, both, np.maximum(snap, np.uint64(floor))), rb)
        want = u.reference(oracle_mod, m, v.table_max())
        assert 0 < int(want.sum()) < len(want)
        np.testing.assert_array_equal(probe(v, m), want)
        u.close()
    print(f"folds: {v.fold_stats()}")
    assert full_joins(v) == before


def union(w, at, lsn):
    """w's rows and rows of keys w.keys[at] + 3 with `lsn`, in key order."""
    keys = np.concatenate([w.keys, w.keys[at] + 3])
    o = np.argsort(keys, kind="stable")
    return Win(keys[o], np.concatenate([w.lsn, lsn])[o])


def test_two_contexts_two_streams(make_validator, oracle_mod):
    """Two windows of the same keys and different commit orders, probed
    alternately on two streams: each context's blocks read its own lists."""
    dev = torch.device("cuda", 0)
    n = 3 * TILE + PARTIAL
    ws = [base_window(), Win(plain_keys(n), distinct_lsns(n, 71))]
    _wins["second"] = ws[1]
    vs = [make_validator(w) for w in ws]
    ms = [cat(w, recent_batch(w, 5000, 72 + k), old_batch(w, 20, 74 + k, tiles=[k + 1])) for k, w in enumerate(ws)]
    want = [w.reference(oracle_mod, m, v.table_max()) for w, v, m in zip(ws, vs, ms)]
    ups = [upload(m) for m in ms]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    outs = [(k % 2, outputs(ms[k % 2])) for k in range(8)]
    torch.cuda.synchronize()
    try:
        for k, (i, out) in enumerate(outs):
            vs[i].set_stream(streams[(k // 2) % 2].cuda_stream)
            launch(vs[i], ms[i], ups[i], out)
        torch.cuda.synchronize()
    finally:
        for v in vs:
            v.set_stream(0)
    for i, (verdict, bits) in outs:
        np.testing.assert_array_equal(result(ms[i], verdict, bits), want[i])
    assert [full_joins(v) for v in vs] == [4, 4]
