"""GPU parity of the narrow join that gives a tile to a wave (k_join_w,
comdb2_amd/csrc/hsc_narrow.hip): a block serves 8 consecutive tiles; a wave
joins its tile when the locate's slot filter kept at most 128 of its records
and every live one can be answered from the tile's recent list, and leaves
any other tile to the whole block, which joins it in the same launch as
k_join_t<true> does.  A block that leaves 3 or more of its 8 tiles sends the
next 64 column batches to k_join_t<true> (hsc_join_stats, include/hip_serial.h).

Windows are built as in test_gpu_join_recent.py: one int64 index ingested as
device rows (LAYOUT_NARROW_TILES), every row a commit of its own, 9 tiles (a
full group of 8 and a group of one, the last tile 777 rows) or 17.  Every
batch is probed with hsc_probe_device into verdict bytes prefilled with 0xFF
and a bitmap of all ones, compared bit for bit with the CPU sort-join, and the
bitmap's bits must equal the verdict bytes.  Every case has a context of its
own.

Records are placed one per range: a point range on a member of a tile's recent
list, at the member's LSN (no conflict) or the LSN before it (a conflict),
survives the filter and can be answered from the list; a point range at a
snapshot after every commit is located and dropped ("filler").  What the
device must do with a batch comes from the numpy models alone: the tiles the
wave kernel leaves to the block are those with more than 128 kept records
(tests/slot_model.py) or a kept record whose snapshot is below the tile's
theta (tests/recent_model.py), and the latter stage the whole tile.

One case of the issue cannot be built: a located record with lo > hi.  The
end-tile step emits a record only for bounds with lo32 <= hi32 (slot_model
`records`: use_a), so no batch reaches the vote with one.  Its nearest
relative is here instead: an old-snapshot record whose bounds hold no row,
which has lo32 <= hi32 and so does fail the vote, with verdict 0.
"""

import numpy as np
import pytest

import recent_model as M
from test_gpu_join_column import batch, paths, probe
from test_gpu_join_recent import (TILE, Win, distinct_lsns, make_validator,  # noqa: F401
                                  plain_keys)
from test_gpu_slot_filter import model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CHUNK = 4096          # probes per locate workgroup: a column entry
WAVE_CAP = 128        # kept records of a tile that one wave joins
WIDE_BLOCK = 3        # tiles of a block's 8 left to the block that make a batch wide
HOT_BATCHES = 64
TILE_CAP = 1024
PARTIAL = 777
NEVER = 1 << 62

_wins = {}


def window(ntiles):
    if ntiles not in _wins:
        n = (ntiles - 1) * TILE + PARTIAL
        _wins[ntiles] = Win(plain_keys(n), distinct_lsns(n, 100 + ntiles))
        assert _wins[ntiles].ntiles == ntiles
    return _wins[ntiles]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for w in _wins.values():
        w.close()
    _wins.clear()


# ---- batches -------------------------------------------------------------------
def members(w, t):
    """Tile t's list members but its first row (a range from a tile's first
    key leaves a record in the tile before as well)."""
    rows = np.asarray(w.lists[t][0])
    return rows[rows != t * TILE]


def kept_points(w, t, k, rng):
    """k records of tile t that survive the filter and stay on its list: (rows, snapshots)."""
    rows = rng.choice(members(w, t), k, replace=True)
    return rows, w.lsn[rows] - (np.arange(k) % 2).astype(np.uint64)


def fillers(w, k, rng, tile=None):
    """k records the filter drops: point ranges at a snapshot after every commit."""
    if tile is None:
        rows = rng.integers(1, len(w.keys), k)
        rows = np.where(rows % TILE == 0, rows + 1, rows)
    else:
        rows = tile * TILE + rng.integers(1, min(TILE, len(w.keys) - tile * TILE), k)
    return rows, np.full(k, w.lsn.max() + np.uint64(1))


def points(w, rows, snap, n_txn=None, txn=None, lock_snap=(), lock_txn=()):
    n = len(rows)
    m = batch(w.keys[rows], w.keys[rows], snap, np.arange(n) if txn is None else txn,
              n if n_txn is None else n_txn, lock_snap, lock_txn)
    m["lo_vals"], m["hi_vals"] = w.keys[rows].copy(), w.keys[rows].copy()
    return m


def per_tile(w, tile_counts, seed):
    """Kept records per tile by `tile_counts` ({tile: k}), in a shuffled order."""
    rng = np.random.default_rng(seed)
    rows, snap = [np.zeros(0, np.int64)], [np.zeros(0, np.uint64)]
    for t, k in tile_counts.items():
        r, s = kept_points(w, t, k, rng)
        rows.append(r), snap.append(s)
    rows, snap = np.concatenate(rows), np.concatenate(snap)
    o = rng.permutation(len(rows))
    return points(w, rows[o], snap[o])


def expect(w, m):
    """By the models: (located, kept) per tile, the tiles k_join_w leaves to
    the block and those of them that stage the whole tile."""
    sm = model(w)
    _, tile, l32, h32, rs = sm.records(m["lo_vals"], m["hi_vals"], m["snap"])
    keep = ~sm.dropped(tile, l32, h32, rs)
    located = np.bincount(tile, minlength=w.ntiles)
    kept = np.bincount(tile[keep], minlength=w.ntiles)
    assert (l32 <= h32).all()
    theta_rank = sm.snap_rank(w.theta)
    old = np.zeros(w.ntiles, bool)
    old[tile[keep & (rs < theta_rank[tile])]] = True
    return located, kept, np.flatnonzero((kept > WAVE_CAP) | old), np.flatnonzero(old)


def stats(v):
    j, b = v.join_stats(), v.batch_stats()
    assert j["wave_batches"] + j["block_batches"] == b["column_batches"]
    return j["wave_batches"], j["block_batches"], j["wave_fallback_tiles"], b["full_tile_joins"]


def run(v, w, oracle_mod, m, kernel="wave", mixed=True, want=None):
    """Probe m (bitmap requested): verdicts equal the sort-join's; on the wave
    kernel the fallback and whole-tile counters rise as the models say.
    Returns the reference verdicts."""
    if want is None:
        want = w.reference(oracle_mod, m, v.table_max())
    if mixed:
        assert 0 < int(want.sum()) < len(want)
    _, _, fall, full = expect(w, m)
    s0 = stats(v)
    got = probe(v, m, bitmap=True)
    v.synchronize()
    s1 = stats(v)
    d = tuple(int(a - b) for a, b in zip(s1, s0))
    print(f"wave/block batches, fallback tiles, full joins: +{d}; model: fallback {list(fall)}, full {list(full)}")
    np.testing.assert_array_equal(got, want)
    if kernel == "wave":
        assert d == (1, 0, len(fall), len(full))
    elif kernel == "block":
        assert d == (0, 1, 0, len(full))
    return want


# ---- kept records of one tile around the wave's capacity ---------------------------
@pytest.mark.parametrize("ntiles", [9, 17])
@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 127, 128, 129])
def test_kept_records_of_one_tile(make_validator, oracle_mod, ntiles, k):
    """Tile 3 keeps exactly k records; its neighbours in the group keep other
    counts (one of them past the capacity), the last tile a few."""
    w = window(ntiles)
    tiles = {0: 5, 1: 130, 2: 0, 3: k, 4: 64, 5: 200, 6: 1, 7: 128, ntiles - 1: 17}
    if ntiles == 17:
        tiles.update({8: 129, 11: 2, 15: 127})
    m = per_tile(w, tiles, seed=1000 + k)
    located, kept, fall, full = expect(w, m)
    np.testing.assert_array_equal(kept, [tiles.get(t, 0) for t in range(ntiles)])
    np.testing.assert_array_equal(located, kept)
    assert len(fall) == sum(x > WAVE_CAP for x in tiles.values()) and len(full) == 0
    v = make_validator(w)
    run(v, w, oracle_mod, m)
    assert paths(v) == (1, 0)


# ---- a tile's records over the chunks of its column -------------------------------
@pytest.mark.parametrize("G", [1, 2, 3])
def test_chunk_runs(make_validator, oracle_mod, G):
    """G chunks of 4096 ranges.  Tile 5 has runs in the first and the last
    chunk and, with G = 3, none in the middle one, where other tiles have
    records; in the last chunk tile 5 is the first tile with a kept record, so
    its run starts at slot 0 of the chunk's area, as tile 0's does in chunk 0.
    Everything else is filler, which the filter drops."""
    w = window(9)
    rng = np.random.default_rng(40 + G)
    n = (G - 1) * CHUNK + 700
    rows, snap = fillers(w, n, rng)
    place = {0: {0: 3, 5: 40, 7: 9}}
    if G == 3:
        place[1] = {2: 30, 6: 11}
    if G > 1:
        place[G - 1] = {5: 50, 8: 20}
    for g, tiles in place.items():
        at = g * CHUNK + rng.permutation(min(CHUNK, n - g * CHUNK))
        for t, k in tiles.items():
            r, s = kept_points(w, t, k, rng)
            rows[at[:k]], snap[at[:k]] = r, s
            at = at[k:]
    m = points(w, rows, snap)
    located, kept, fall, full = expect(w, m)
    assert kept[5] == (90 if G > 1 else 40) and kept.max() <= WAVE_CAP and located.sum() == n
    assert len(fall) == 0
    v = make_validator(w)
    run(v, w, oracle_mod, m)
    assert paths(v) == (1, 0)


# ---- ranges of many list rows ----------------------------------------------------------
def test_long_ranges(make_validator, oracle_mod):
    """A lane reads a range of up to four list rows itself and leaves longer
    ones to the wave's passes: 60 ranges per tile of 1 to 3000 rows (0 to
    about 190 list rows), each at the newest LSN inside or the one before,
    raised to the tile's theta so that the list can answer."""
    w = window(9)
    rng = np.random.default_rng(55)
    tiles = np.repeat(np.arange(9), 60)
    rows = np.minimum(TILE, len(w.keys) - tiles * TILE)
    ln = np.minimum(rng.choice([1, 2, 5, 17, 33, 64, 100, 260, 700, 3000], len(tiles)), rows - 1)
    pa = tiles * TILE + 1 + rng.integers(0, 1 << 30, len(tiles)) % (rows - ln)
    pb = pa + ln
    newest = M.range_max(w.lsn.astype(np.int64), pa, pb).astype(np.uint64)
    snap = np.maximum(newest - rng.integers(0, 2, len(tiles)).astype(np.uint64), w.theta[tiles])
    o = rng.permutation(len(tiles))
    m = batch(w.keys[pa][o], w.keys[pb - 1][o], snap[o], np.arange(len(tiles)), len(tiles))
    m["lo_vals"], m["hi_vals"] = w.keys[pa][o], w.keys[pb - 1][o]
    _, kept, fall, _ = expect(w, m)
    assert 30 <= kept.min() and kept.max() <= 60 and len(fall) == 0
    nlist = np.array([np.isin(np.arange(a, b), w.lists[t][0]).sum() for a, b, t in zip(pa, pb, tiles)])
    assert (nlist <= 4).sum() > 100 and (nlist > 4).sum() > 100 and nlist.max() > 128
    v = make_validator(w)
    run(v, w, oracle_mod, m)
    assert paths(v) == (1, 0)


# ---- the vote ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["row", "no-row"])
def test_vote_failure(make_validator, oracle_mod, kind):
    """One record of tile 4 has a snapshot below the tile's theta: on a row
    left out of the list (a conflict only the whole tile shows), or between
    two keys (bounds that hold no row: lo32 <= hi32 still, so the vote fails
    all the same and the answer is 0).  That tile falls back and stages
    whole; the other seven stay with their waves."""
    w = window(9)
    m = per_tile(w, {t: 20 + t for t in range(9)}, seed=7)
    out = w.out_rows(4, first=False)
    row = out[np.argmax(w.lsn[out])]  # the cut: its LSN is theta
    assert w.lsn[row] == w.theta[4]
    lo = w.keys[row] + (1 if kind == "no-row" else 0)
    hi = w.keys[row] + (3 if kind == "no-row" else 0)
    m2 = batch(np.append(m["lo_vals"], lo), np.append(m["hi_vals"], hi),
               np.append(m["snap"], w.lsn[row] - np.uint64(1)), np.arange(m["n"] + 1), m["n"] + 1)
    m2["lo_vals"], m2["hi_vals"] = np.append(m["lo_vals"], lo), np.append(m["hi_vals"], hi)
    _, kept, fall, full = expect(w, m2)
    assert kept[4] == 25 and list(fall) == [4] and list(full) == [4]
    v = make_validator(w)
    want = run(v, w, oracle_mod, m2)
    assert bool(want[-1]) == (kind == "row")
    # without that record nothing falls back
    v2 = make_validator(w)
    assert len(expect(w, m)[2]) == 0
    run(v2, w, oracle_mod, m)


# ---- the wide rule ------------------------------------------------------------------
def test_wide_batches(make_validator, oracle_mod):
    """17 tiles: groups 0-7, 8-15 and 16.  Batches with 0, 1 and 2 tiles past
    the capacity in the first group -- the last with 2 more in the second, 4
    in all but no block with 3 -- keep the next batch on the wave kernel; 3 in
    one group send the next 64 to k_join_t<true>, the 65th is back."""
    w = window(17)
    v = make_validator(w)
    base = {t: 10 + 3 * t for t in range(17)}
    over = [base, {**base, 2: 129}, {**base, 2: 129, 7: 300, 9: 129, 15: 140},
            {**base, 0: 129, 3: 150, 6: 131}]
    ms = [per_tile(w, tiles, seed=300 + i) for i, tiles in enumerate(over)]
    for m, nfall in zip(ms, (0, 1, 4, 3)):
        assert len(expect(w, m)[2]) == nfall
        run(v, w, oracle_mod, m)  # (asserts: joined by the wave kernel)
    cool = ms[0]
    want = w.reference(oracle_mod, cool, v.table_max())
    for k in range(HOT_BATCHES):
        run(v, w, oracle_mod, ms[k % 4] if k < 4 else cool, kernel="block", want=None if k < 4 else want)
    run(v, w, oracle_mod, cool, want=want)
    assert stats(v)[:2] == (5, HOT_BATCHES) and paths(v) == (5 + HOT_BATCHES, 0)


# ---- the hot rule -------------------------------------------------------------------
def test_hot_rule_on_the_wave_kernel(make_validator, oracle_mod):
    """1200 fillers into tile 2 and a few kept records everywhere: tile 2 is
    given more than 1024 located records and keeps 30.  The wave kernel joins
    the batch; the next one takes the plan path, as it does with k_join_t<true>."""
    w = window(9)
    rng = np.random.default_rng(81)
    m0 = per_tile(w, {t: 30 for t in range(9)}, seed=82)
    fr, fs = fillers(w, 1200, rng, tile=2)
    o = rng.permutation(m0["n"] + 1200)
    rows = np.concatenate([np.searchsorted(w.keys, m0["lo_vals"]), fr])[o]
    m = points(w, rows, np.concatenate([m0["snap"], fs])[o])
    located, kept, fall, _ = expect(w, m)
    assert located[2] == 1230 > TILE_CAP and kept[2] == 30 and len(fall) == 0
    v = make_validator(w)
    run(v, w, oracle_mod, m)
    assert paths(v) == (1, 0)
    run(v, w, oracle_mod, m0, kernel="plan")
    assert paths(v) == (1, 1) and stats(v)[:2] == (1, 0)


# ---- the flag move ------------------------------------------------------------------
def test_flag_move(make_validator, oracle_mod):
    """9 tiles: a grid of 8 blocks, 6 of them with no tile, 4096 threads.
    200,000 read sets: every second one holds a table lock, half of those at a
    snapshot before every commit (the locate flags them); 300 hold a range.
    Every flag arrives in its verdict byte and bitmap bit; the same batch at
    snapshots after every commit then gives all zeros, so no flag was left."""
    w = window(9)
    n_txn = 200_000
    m0 = per_tile(w, {t: 30 + t for t in range(9)}, seed=91)
    rng = np.random.default_rng(92)
    odd = np.arange(1, n_txn, 2)
    txn = rng.choice(odd, m0["n"], replace=False)
    lock_txn = np.arange(0, n_txn, 2)
    before = np.uint64(int(w.lsn.min()) - 1)
    lock_snap = np.where(lock_txn % 4 == 0, before, np.uint64(NEVER))
    rows = np.searchsorted(w.keys, m0["lo_vals"])
    m = points(w, rows, m0["snap"], n_txn, txn, lock_snap, lock_txn)
    v = make_validator(w)
    want = run(v, w, oracle_mod, m)
    assert want[lock_txn[lock_txn % 4 == 0]].all() and not want[lock_txn[lock_txn % 4 == 2]].any()
    quiet = points(w, rows, np.full(len(rows), np.uint64(NEVER)), n_txn, txn,
                   np.full(len(lock_txn), np.uint64(NEVER)), lock_txn)
    assert not run(v, w, oracle_mod, quiet, mixed=False).any()
    assert stats(v)[:2] == (2, 0)
