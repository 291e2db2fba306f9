"""The slot filter's model (tests/slot_model.py) against brute force: on random
windows and batches no record the rule drops has a row inside its bounds that
is newer than its snapshot -- with the table exact (qshift = 0) and quantised
(qshift > 0) -- and the rule does drop records (the kept count is printed).
Config 2's generator at a reduced size reports the share of join records the
filter keeps.
"""

import numpy as np
import pytest

import slot_model as S
from comdb2_amd.workloads import config2

TILE = S.TILE


def random_window(rng, ntiles, partial, gap_bits, lsn_span):
    n = (ntiles - 1) * TILE + partial
    keys = np.cumsum(rng.integers(1, 1 << gap_bits, n, dtype=np.int64)) + 12345
    lsn = np.uint64(7 << 32) + rng.integers(0, lsn_span, n).astype(np.uint64)
    return keys, lsn


def random_batch(rng, keys, lsn, n):
    """Narrow ranges around rows (some empty, some over a tile edge), snapshots
    near the newest row inside or anywhere in the window's span."""
    r0 = rng.integers(0, len(keys), n)
    k = rng.integers(0, 30, n)
    r1 = np.minimum(r0 + k, len(keys) - 1)
    lo = keys[r0] - rng.integers(0, 3, n)
    hi = keys[r1] + rng.integers(0, 3, n)
    newest = np.array([lsn[a:b + 1].max() for a, b in zip(r0, r1)])
    anyw = lsn[rng.integers(0, len(lsn), n)]
    snap = np.where(rng.random(n) < 0.7, newest - rng.integers(0, 3, n).astype(np.uint64), anyw)
    snap[rng.random(n) < 0.05] = lsn.max() + np.uint64(1)  # after every row: droppable whatever the slots
    return lo, hi, snap


@pytest.mark.parametrize("ntiles, partial, gap_bits, lsn_span, qshift", [
    (4, 777, 3, 50_000, 0),         # dense keys, exact table
    (4, 777, 19, 60_000, 0),        # keys up to 2^19 apart: tiles span 2^30
    (3, 1, 10, 1 << 24, 8),         # quantised: 256 LSNs a quantum
    (5, 4095, 16, 1 << 31, 15),
    (1, 300, 2, 1000, 0),           # one short tile: shift from span 2^32
])
def test_no_dropped_record_has_a_newer_row(ntiles, partial, gap_bits, lsn_span, qshift):
    rng = np.random.default_rng([ntiles, partial, gap_bits])
    keys, lsn = random_window(rng, ntiles, partial, gap_bits, lsn_span)
    w = S.SlotWindow(keys, lsn)
    assert w.filters and w.qshift == qshift
    lo, hi, snap = random_batch(rng, keys, lsn, 4000)
    _, tile, l32, h32, rs = w.records(lo, hi, snap)
    drop = w.dropped(tile, l32, h32, rs)
    newer = w.newer_row_inside(tile, l32, h32, rs)
    print(f"records {len(tile)}, kept {int((~drop).sum())}, with a newer row {int(newer.sum())}")
    assert not (drop & newer).any()
    assert drop.any() and newer.any()
    if qshift == 0:
        # exact entries: a record inside one slot is kept only for a row of that
        # slot at or after r(S)
        sh = w.shift[tile]
        one = (l32 >> sh) == (h32 >> sh)
        s = np.minimum(l32 >> sh, S.SLOTS - 1)
        np.testing.assert_array_equal(drop[one], (w.table[tile, s] < rs)[one])
    # a coarser table stays sound
    wq = S.SlotWindow(keys, lsn, qshift=w.qshift + 3)
    dq = wq.dropped(tile, l32, h32, rs)
    assert not (dq & newer).any() and not (dq & ~drop).any()


def test_slot_shift():
    for span in (1, 2, 511, 512, 513, 1024, 1025, (1 << 20) + 1, 1 << 32, (1 << 32) - 1):
        s = S.slot_shift(span)
        assert (span - 1) >> s < S.SLOTS and (s == 0 or (span - 1) >> (s - 1) >= S.SLOTS)
    assert S.slot_shift(1 << 32) == 23 and S.slot_shift(512) == 0 and S.slot_shift(513) == 1
    assert [S.qshift_of(r) for r in (1, 65535, 65536, 1 << 20, 0xFFFFFFFF)] == [0, 0, 1, 5, 16]


def test_general_windows_drop_nothing():
    rng = np.random.default_rng(3)
    keys, _ = random_window(rng, 2, 100, 4, 10)
    lsn = np.uint64(5 << 32) + (1 + rng.permutation(len(keys)).astype(np.uint64)) * np.uint64(1 << 21)
    w = S.SlotWindow(keys, lsn)
    assert not w.filters
    located, kept = w.kept(*random_batch(rng, keys, lsn, 2000))
    assert located == kept > 0


def config2_bounds(c2, keys):
    """Config 2's ranges as int64 bounds over the window `keys`: prefix ranges
    cover the values sharing the prefix, an open side ends at the window's."""
    rs = c2.readsets
    b = rs.keys.reshape(-1, 9)
    nr = len(rs.lflag)
    val = lambda rows: (rows[:, 1:].copy().view(">u8").reshape(-1).astype(np.uint64)
                        ^ np.uint64(1 << 63)).view(np.int64)
    lo, hi = val(b[:nr]), val(b[nr:])
    ml = (np.int64(1) << (8 * (9 - rs.lkeylen.astype(np.int64)))) - 1
    mh = (np.int64(1) << (8 * (9 - rs.rkeylen.astype(np.int64)))) - 1
    lo = np.where(rs.lflag == 1, keys[0], lo & ~ml)
    hi = np.where(rs.rflag == 1, keys[-1], hi | mh)
    return lo, hi, np.repeat(rs.snap, np.diff(rs.txn_off))


@pytest.mark.parametrize("snap_recent", [0.01, 1.0])
def test_config2_kept_share(snap_recent):
    """Config 2 at 1/20 of its size (the key space narrowed with it, so a range
    meets as many rows).  At snap_recent 0.01 the filter must leave a minority
    of the records; at 1.0 (old snapshots) it can drop few."""
    c2 = config2(n_commits=50_000, n_txn=5_000, value_bits=36, width=1 << 20, snap_recent=snap_recent,
                 build_log=False)
    lsn = np.repeat(c2.commit_lsn, 10)
    o = np.lexsort((lsn, c2.key_values))
    k, l = c2.key_values[o], lsn[o]
    last = np.append(k[1:] != k[:-1], True)  # a key's newest version
    w = S.SlotWindow(k[last], l[last])
    assert w.filters
    lo, hi, snap = config2_bounds(c2, w.keys)
    _, tile, l32, h32, rs = w.records(lo, hi, snap)
    drop = w.dropped(tile, l32, h32, rs)
    share = float((~drop).mean())
    print(f"config 2 / 20, snap_recent {snap_recent}: qshift {w.qshift}, {len(tile)} join records, "
          f"kept {int((~drop).sum())} ({100 * share:.1f} %)")
    sel = np.random.default_rng(1).choice(len(tile), 3000, replace=False)
    newer = w.newer_row_inside(tile[sel], l32[sel], h32[sel], rs[sel])
    assert not (drop[sel] & newer).any()
    assert share < 0.5 if snap_recent < 1 else share > 0.5
