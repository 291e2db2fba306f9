"""The recent lists' exactness rule on the numpy model (tests/recent_model.py):
for every threshold rs >= theta a range's answer over the list members is its
answer over the whole tile, and at rs = theta - 1 it is not, so theta is the
least bound that holds -- a test can place a snapshot on either side of it.
Tiles of 4096 rows with heavy ties: 10 rows per commit, and all rows on 3
ranks.  No GPU."""

import numpy as np
import pytest

import recent_model as M


def tile_ten_per_commit(seed):
    """The newest commit has 9 rows: the cut (256 = 9 + 24 * 10 + 7) splits a commit's rows."""
    rng = np.random.default_rng(seed)
    return 1 + (rng.permutation(M.TILE) + 3) // 10


def tile_three_ranks(seed):
    rng = np.random.default_rng(seed)
    return np.array([5, 9, 14])[rng.integers(0, 3, M.TILE)]


def sampled_ranges(seed):
    """Every point range, every range of 17 rows, 3000 random ones, the whole
    tile and the empty range."""
    rng = np.random.default_rng(seed)
    i = np.arange(M.TILE)
    a = rng.integers(0, M.TILE, 3000)
    b = np.minimum(M.TILE, a + 1 + rng.integers(0, 1 << rng.integers(1, 12, 3000)))
    pa = np.concatenate([i, i[:-17], a, [0, 7]])
    pb = np.concatenate([i + 1, i[:-17] + 17, b, [M.TILE, 7]])
    return pa, pb


TILES = [(f, s) for f in (tile_ten_per_commit, tile_three_ranks) for s in (1, 2, 3)]


@pytest.mark.parametrize("make,seed", TILES, ids=[f"{f.__name__}-{s}" for f, s in TILES])
def test_list_answers_for_every_threshold_from_theta(make, seed):
    rank = make(seed)
    members, theta = M.tile_list(rank)
    assert len(members) == M.R and theta >= 1
    # the list is the newest rows, ties at the cut to the earlier row
    out = np.setdiff1d(np.arange(M.TILE), members)
    assert rank[members].min() >= theta == rank[out].max()
    tie_in, tie_out = members[rank[members] == theta], out[rank[out] == theta]
    assert len(tie_out) > 0
    if len(tie_in):
        assert tie_in.max() < tie_out.min()
    pa, pb = sampled_ranges(seed)
    rs = np.concatenate([np.unique(rank[rank >= theta]), [theta, int(rank.max()) + 1]])
    np.testing.assert_array_equal(M.list_answer(rank, members, pa, pb, rs), M.full_answer(rank, pa, pb, rs))
    # one below theta: a row left out commits after the snapshot, the list misses it
    below = [theta - 1]
    assert (M.list_answer(rank, members, pa, pb, below) != M.full_answer(rank, pa, pb, below)).any()


@pytest.mark.parametrize("tn", [1, 255, 256, 257, 1000])
def test_short_tiles(tn):
    rank = 1 + np.random.default_rng(tn).permutation(tn)
    members, theta = M.tile_list(rank)
    assert len(members) == min(M.R, tn)
    if tn <= M.R:
        assert theta == 0 and np.array_equal(members, np.arange(tn))
    else:
        assert theta == tn - M.R  # ranks are 1 .. tn: the newest 256 are in
    i = np.arange(tn)
    rs = np.arange(theta, tn + 2)
    np.testing.assert_array_equal(M.list_answer(rank, members, i, i + 1, rs), M.full_answer(rank, i, i + 1, rs))


def test_window_lists_split_by_tile():
    rank = 1 + np.random.default_rng(7).permutation(2 * M.TILE + 300)
    lists = M.window_lists(rank)
    assert [len(m) for m, _ in lists] == [M.R, M.R, M.R]
    for t, (m, th) in enumerate(lists):
        assert (m // M.TILE == t).all()
        tile = rank[t * M.TILE:(t + 1) * M.TILE]
        assert th == np.sort(tile)[-M.R - 1]
    np.testing.assert_array_equal(M.thetas(rank), [th for _, th in lists])
