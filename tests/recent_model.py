"""A numpy model of the narrow tiles' recent lists (k_recent,
comdb2_amd/csrc/hsc_narrow.hip).

A window is rows in key order with a commit time each (an LSN, or a rank: any
unsigned values whose order is the commits'); tile t holds rows 4096 t ..
4096 t + tn - 1.  Per tile:

  members  the min(R, tn) rows with the largest commit time, R = 256; ties at
           the cut go to the smaller key, i.e. the earlier row;
  theta    the largest commit time of a row left out, 0 when none is (commit
           times are >= 1).

The rule the join relies on: for a snapshot S >= theta every row of the tile
committed after S is a member, so a range's answer over the members alone
("some member inside the range committed after S") is its answer over the
whole tile.
"""

import numpy as np

TILE = 4096
R = 256


def tile_list(rank):
    """(members, theta) of one tile: `rank` = its rows' commit times in key
    order; members = their row numbers in the tile, ascending."""
    rank = np.asarray(rank, np.uint64)
    tn = len(rank)
    if tn <= R:
        return np.arange(tn), 0
    # newest first, ties by row: a stable sort of the negated order
    order = np.argsort(-rank.astype(np.int64), kind="stable")
    members = np.sort(order[:R])
    return members, int(rank[order[R:]].max())


def window_lists(rank, tile=TILE):
    """[(members as window row numbers, theta)] per tile of a window."""
    rank = np.asarray(rank, np.uint64)
    out = []
    for a in range(0, len(rank), tile):
        m, th = tile_list(rank[a:a + tile])
        out.append((a + m, th))
    return out


def thetas(rank, tile=TILE):
    return np.array([th for _, th in window_lists(rank, tile)], np.uint64)


def range_max(v, pa, pb):
    """max v[pa:pb) per pair, 0 for an empty range (v >= 0)."""
    v = np.asarray(v, np.int64)
    pa, pb = np.asarray(pa, np.int64), np.asarray(pb, np.int64)
    levels = [v]
    while (1 << len(levels)) <= len(v):
        m, h = levels[-1], 1 << (len(levels) - 1)
        levels.append(np.maximum(m[:-h], m[h:]))
    out = np.zeros(len(pa), np.int64)
    live = pb > pa
    lv = np.zeros(len(pa), np.int64)
    lv[live] = np.floor(np.log2((pb - pa)[live])).astype(np.int64)
    for l in np.unique(lv[live]):
        s = live & (lv == l)
        m = levels[l]
        out[s] = np.maximum(m[pa[s]], m[pb[s] - (1 << int(l))])
    return out


def full_answer(rank, pa, pb, rs):
    """Rows [pa, pb) of a tile hold one with rank > rs (per range and threshold: [ranges, thresholds])."""
    return range_max(rank, pa, pb)[:, None] > np.asarray(rs, np.int64)[None, :]


def list_answer(rank, members, pa, pb, rs):
    """The same asked of the members only."""
    only = np.zeros(len(rank), np.int64)
    only[members] = np.asarray(rank, np.int64)[members]
    return range_max(only, pa, pb)[:, None] > np.asarray(rs, np.int64)[None, :]
