"""GPU parity of the locate's slot filter, the located-record hot rule and the
join's dealt rounds (k_recent, k_locate_t, k_plan_s, join_s_item,
comdb2_amd/csrc/hsc_narrow.hip).

Windows are built as in test_gpu_join_recent.py: one int64 index ingested as
device rows (LAYOUT_NARROW_TILES), three full 4096-row tiles and one of 777
rows unless a case says otherwise, commit LSNs spanning < 2^32.  Every batch
is probed with hsc_probe_device into verdict bytes prefilled with 0xFF and
compared bit for bit with the CPU sort-join; the number of join records that
survive the filter (hsc_get_timing's `records`: the sum of the tiles' kept
counts) must equal the numpy model's (tests/slot_model.py) exactly.  Without
the filter that count is the located one, which every filtering case asserts
to be larger.

One case of the issue cannot exist: a tile whose span is under 512 codes
(shift 0).  A tile's span is the distance to the next tile's first code, every
tile but the last holds 4096 distinct codes, and the last one's span is 2^32
by definition, so the smallest span is 4096 (shift 3): `dense` below.
"""

import numpy as np
import pytest

import appended_model as A
import recent_model as M
import slot_model as S
from comdb2_amd.hsc import PATH_NO_SMALL
from comdb2_amd.workloads import int64_words
from test_gpu_appended_placed import append
from test_gpu_join_column import paths, probe
from test_gpu_join_recent import (KEY0, LSN0, PARTIAL, TILE, Win, distinct_lsns, make_batch,  # noqa: F401
                                  make_validator, plain_keys, ranges, skewed_window, union)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE_CAP = 1024
HOT_BATCHES = 64
N = 3 * TILE + PARTIAL


def model(w):
    if getattr(w, "slots", None) is None:
        w.slots = S.SlotWindow(w.keys, w.lsn)
    return w.slots


def counts(w, m, general=False):
    """(located, kept) per tile by the model; a general locate instance keeps all."""
    sm = model(w)
    _, tile, l32, h32, rs = sm.records(m["lo_vals"], m["hi_vals"], m["snap"])
    located = np.bincount(tile, minlength=w.ntiles)
    if general:
        return located, located
    return located, np.bincount(tile[~sm.dropped(tile, l32, h32, rs)], minlength=w.ntiles)


def run(v, w, oracle_mod, m, general=False, mixed=True):
    """Probe m: verdicts equal the sort-join's, the surviving records the model's.
    Returns (located, kept) per tile."""
    want = w.reference(oracle_mod, m, v.table_max())
    if mixed:
        assert 0 < int(want.sum()) < len(want)
    located, kept = counts(w, m, general)
    got = probe(v, m)
    v.synchronize()
    records = v.timing()["records"]
    print(f"located {int(located.sum())}, kept by the model {int(kept.sum())}, by the device {records}")
    np.testing.assert_array_equal(got, want)
    assert records == int(kept.sum())
    return located, kept


@pytest.fixture
def timed(make_validator):
    def make(w, **kw):
        v = make_validator(w, **kw)
        v.enable_timing(True)
        return v
    return make


def edge_batch(w, tiles=None, nslots=(1, 2, 3)):
    """Per tile and a sample of its slots s: ranges from one below, on and one
    above slot s's first code to one below, on and one above the last code of
    slot s + k - 1, k in nslots, each at snapshots around the largest rank M of
    those slots' rows: M - 1, M, M + 1 and, with a quantum Q = 2^qshift > 1,
    the ends of M's quantum and the ranks just outside it."""
    sm = model(w)
    Q = 1 << sm.qshift
    lo, hi, snap = [], [], []
    for t in range(sm.ntiles) if tiles is None else tiles:
        sh = int(sm.shift[t])
        used = np.unique(sm.slot[t * TILE:(t + 1) * TILE])
        pick = np.unique(np.concatenate([used[:3], used[len(used) // 2:len(used) // 2 + 2], used[-2:], [0, 510]]))
        for s in pick:
            for k in nslots:
                M = max(int(sm.smax[t, s:s + k].max()), 2)
                offs = {-1, 0, 1}
                if Q > 1:
                    offs |= {-(M % Q) - 1, -(M % Q), Q - 1 - (M % Q), Q - (M % Q)}
                for a in (-1, 0, 1):
                    for b in (-1, 0, 1):
                        clo = int(sm.first[t]) + (int(s) << sh) + a
                        chi = int(sm.first[t]) + ((int(s) + k) << sh) - 1 + b
                        if clo < 0 or chi < clo:
                            continue
                        for o in sorted(offs):
                            if M + o < 1:
                                continue
                            lo.append(int(w.keys[0]) + (clo << sm.tz))
                            hi.append(int(w.keys[0]) + (chi << sm.tz))
                            snap.append(sm.base + M + o - 1)
    return make_batch(w, np.array(lo, np.int64), np.array(hi, np.int64), np.array(snap, np.uint64))


def base_window():
    return Win(plain_keys(N), distinct_lsns(N, 11))


# ---- (i) - (iii): slot edges, slot shapes, quantised maxima ----------------------
def one_tile():
    return Win(plain_keys(1000), distinct_lsns(1000, 12))


def dense():
    """Consecutive keys: every full tile spans exactly 4096 codes, the smallest span there is."""
    return Win(KEY0 + np.arange(N, dtype=np.int64), distinct_lsns(N, 13))


def quantised():
    """LSNs 2^17 apart: the largest rank needs qshift = 15."""
    return Win(plain_keys(N), distinct_lsns(N, 14, 1 << 17))


SHAPES = {
    # base: tiles of span 4096 * 7 (shift 6), the partial last tile with span 2^32 (shift 23)
    "base": (base_window, 0, 0),
    "one-tile": (one_tile, 0, 0),
    "dense": (dense, 0, 0),
    # 12 dense tiles and 8 of keys 2^20 apart (a span of 2^32, clamped): the
    # bucket table takes log mode, so this is the kLocFastLog instance on the plan path
    "keys-2^20-apart": (skewed_window, 1, 1),  # (78,601 rows, a commit each: qshift 1)
    "quantised": (quantised, 15, 0),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_slot_edges(timed, oracle_mod, shape):
    make, qshift, plan = SHAPES[shape]
    w = make()
    try:
        sm = model(w)
        assert sm.filters and sm.qshift == qshift
        if shape == "dense":
            assert (sm.shift[:-1] == 3).all() and sm.shift[-1] == 23
        if shape == "keys-2^20-apart":
            assert (sm.shift[-8:] == 23).all()
        v = timed(w)
        tiles = None if w.ntiles <= 4 else [0, 5, 11, 12, 15, w.ntiles - 1]
        m = edge_batch(w, tiles)
        located, kept = run(v, w, oracle_mod, m)
        assert 0 < kept.sum() < located.sum()
        assert paths(v) == ((0, 1) if plan else (1, 0))
        assert v.batch_stats()["fast_locates"] == 1
        # ranges that reach three slots or more are never dropped
        m3 = edge_batch(w, tiles, nslots=(3,))
        _, tile3, l3, h3, rs3 = sm.records(m3["lo_vals"], m3["hi_vals"], m3["snap"])
        sh3 = sm.shift[tile3]
        wide = np.minimum(h3 >> sh3, S.SLOTS - 1) - np.minimum(l3 >> sh3, S.SLOTS - 1) >= 2
        assert wide.any() and not sm.dropped(tile3, l3, h3, rs3)[wide].any()
    finally:
        w.close()


# ---- (iv) folds: the folded window's table is new --------------------------------
@pytest.mark.parametrize("background", [False, True], ids=["inline", "background"])
def test_fold_rebuilds_the_table(timed, oracle_mod, background):
    """750 rows appended in three pieces, keys between the window's, each newer
    than every row before; a fold at 600 rows.  After every piece and after
    the last fold every appended row is probed at its LSN - 1 (a conflict) and
    at its LSN (none): a table older than the folded window would drop the
    conflicts.  Once nothing is left in the run the kept count is the folded
    window's."""
    w = base_window()
    v = timed(w, fold=(600, background), path_flags=PATH_NO_SMALL)
    rng = np.random.default_rng(61)
    at = np.sort(rng.choice(N - 1, 750, replace=False))
    order = rng.permutation(750)
    end = int(w.lsn.max()) + 1
    app = A.Rows(np.zeros(750, np.uint32), int64_words(w.keys[at] + 3), np.uint64(end) + order.astype(np.uint64))
    done = np.zeros(750, bool)
    try:
        for piece in range(4):
            if piece < 3:
                sel = np.flatnonzero(order // 250 == piece)
                sel = sel[np.argsort(order[sel])]
                append(v, app.take(sel))
                done[sel] = True
                if not background and v.delta_rows >= 600:
                    v.export_window()
            else:
                v.export_window()
                assert v.delta_rows == 0
            u = union(w, at[done], app.lsn[done])
            rows = np.flatnonzero(u.lsn >= end)
            m = make_batch(u, np.tile(u.keys[rows], 2), np.tile(u.keys[rows], 2),
                           np.concatenate([u.lsn[rows] - np.uint64(1), u.lsn[rows]]))
            want = u.reference(oracle_mod, m, v.table_max())
            np.testing.assert_array_equal(want, np.arange(m["n"]) < len(rows))
            got = probe(v, m)
            v.synchronize()
            np.testing.assert_array_equal(got, want)
            if v.delta_rows == 0 and (piece == 3 or not background):
                assert v.timing()["records"] == int(counts(u, m)[1].sum())
            u.close()
        print(f"folds: {v.fold_stats()}")
    finally:
        w.close()


# ---- (v) the general instances drop nothing ----------------------------------------
GENERAL = {
    # commits 2^21 apart span >= 2^32: ranks from the commit directory
    "directory-ranks": lambda: Win(plain_keys(N), distinct_lsns(N, 42, 1 << 21)),
    # one-word keys over a log-mode table: no fast instance
    "log-mode-one-word": lambda: Win(skewed_window().keys, distinct_lsns(19 * TILE + PARTIAL, 43), words=1),
}


@pytest.mark.parametrize("mode", list(GENERAL))
def test_general_instances(timed, oracle_mod, mode):
    w = GENERAL[mode]()
    try:
        sm = model(w)
        assert sm.filters == (mode != "directory-ranks")
        v = timed(w)
        tiles = None if w.ntiles <= 4 else [0, 5, 12, w.ntiles - 1]
        m = edge_batch(w, tiles)
        located, kept = run(v, w, oracle_mod, m, general=True)
        np.testing.assert_array_equal(located, kept)
        if sm.filters:  # a fast instance would have dropped some of these
            assert counts(w, m)[1].sum() < located.sum()
        st = v.batch_stats()
        assert (st["fast_locates"], st["general_locates"]) == (0, 1)
    finally:
        w.close()


# ---- (vi) the hot rule counts located records ----------------------------------------
def dropped_batch(w, tile, n, seed):
    """n ranges of one to four rows inside `tile` (at most two slots each)
    whose snapshot is after every commit -- the model drops each -- and 300
    over all tiles at the newest LSN inside or the one before."""
    rng = np.random.default_rng(seed)
    r0 = tile * TILE + rng.integers(1, TILE - 8, n)
    lo, hi = w.keys[r0], w.keys[r0 + rng.integers(0, 4, n)]
    l2, h2, newest = ranges(w, np.arange(300) % w.ntiles, seed + 1)
    s2 = newest - rng.integers(0, 2, 300).astype(np.uint64)
    return make_batch(w, np.concatenate([lo, l2]), np.concatenate([hi, h2]),
                      np.concatenate([np.full(n, w.lsn.max() + np.uint64(1)), s2]))


def balanced_batch(w, n, seed):
    lo, hi, newest = ranges(w, np.arange(n) % w.ntiles, seed)
    return make_batch(w, lo, hi, newest - np.random.default_rng(seed).integers(0, 2, n).astype(np.uint64))


def test_hot_rule_counts_located_records(timed, oracle_mod):
    """1200 ranges into tile 2, every one dropped: the tile keeps under a
    hundred records and still sends the next batches down the plan path; the
    same batch met on the plan path renews the 64 batches from there."""
    w = base_window()
    try:
        v = timed(w)
        hot = dropped_batch(w, 2, 1200, 81)
        located, kept = counts(w, hot)
        assert located[2] >= 1200 > TILE_CAP > kept.max() and kept[2] <= 100
        run(v, w, oracle_mod, hot)
        assert paths(v) == (1, 0)
        run(v, w, oracle_mod, hot)        # batch 2, on the plan path: hot again
        assert paths(v) == (1, 1)
        cool = balanced_batch(w, 2000, 82)
        assert counts(w, cool)[0].max() <= TILE_CAP
        for k in range(HOT_BATCHES):     # batches 3 .. 66: within 64 of batch 2
            run(v, w, oracle_mod, cool)
            assert paths(v) == (1, 2 + k)
        run(v, w, oracle_mod, cool)      # batch 67
        assert paths(v) == (2, 1 + HOT_BATCHES)
    finally:
        w.close()


def test_balanced_batch_stays_on_the_column_path(timed, oracle_mod):
    """5000 ranges over 8 tiles, 625 located records each."""
    n = 7 * TILE + PARTIAL
    w = Win(plain_keys(n), distinct_lsns(n, 83))
    try:
        v = timed(w)
        m = balanced_batch(w, 5000, 84)
        assert counts(w, m)[0].max() <= TILE_CAP
        for k in range(3):
            run(v, w, oracle_mod, m)
            assert paths(v) == (k + 1, 0)
    finally:
        w.close()


# ---- (vii) dealt rounds -----------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025])
def test_dealt_rounds(timed, oracle_mod, k):
    """Tile 2 given exactly k surviving records (snapshots alternate between
    the newest LSN inside the range and the one before; either keeps its
    record: a tie with the slot maximum is no drop), on the column path and,
    after a batch that makes the context hot, on the plan path, where records
    past 1024 go to an overflow item."""
    w = base_window()
    try:
        # (off the tile's first row: a range from it leaves a record in the tile before)
        rng = np.random.default_rng(90 + k)
        pa = 2 * TILE + 1 + rng.integers(0, TILE - 50, k)
        pb = pa + rng.integers(0, 40, k) + 1
        lo, hi = w.keys[pa], w.keys[pb - 1]
        newest = M.range_max(w.lsn.astype(np.int64), pa, pb).astype(np.uint64)
        m = make_batch(w, lo, hi, newest - (np.arange(k) % 2).astype(np.uint64))
        located, kept = counts(w, m)
        assert kept[2] == k == kept.sum()
        v = timed(w)
        run(v, w, oracle_mod, m, mixed=k > 1)
        assert paths(v) == (1, 0)
        v2 = timed(w)
        run(v2, w, oracle_mod, dropped_batch(w, 1, 1200, 91))
        run(v2, w, oracle_mod, m, mixed=k > 1)
        assert paths(v2) == (1, 1)
    finally:
        w.close()


def test_far_snapshot_keeps_wide_ranges(timed, oracle_mod):
    """Snapshots far past the window give r(S) >> qshift above every u16 entry:
    ranges inside two slots are dropped, ranges reaching three or more go on
    to the join all the same (the filter never looked at their slots)."""
    w = quantised()
    try:
        sm = model(w)
        m = edge_batch(w)
        far = np.arange(m["n"]) % 2 == 0
        m["snap"] = np.where(far, w.lsn.max() + np.uint64(1 << 33), m["snap"])
        _, tile, l32, h32, rs = sm.records(m["lo_vals"], m["hi_vals"], m["snap"])
        assert ((rs >> sm.qshift) > 0xFFFF).any()
        sh = sm.shift[tile]
        wide = np.minimum(h32 >> sh, S.SLOTS - 1) - np.minimum(l32 >> sh, S.SLOTS - 1) >= 2
        drop = sm.dropped(tile, l32, h32, rs)
        assert (wide & ((rs >> sm.qshift) > 0xFFFF)).any() and not drop[wide].any() and drop.any()
        run(timed(w), w, oracle_mod, m)
    finally:
        w.close()
