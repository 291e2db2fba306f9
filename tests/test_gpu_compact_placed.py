"""GPU: placed probes of the compact-code bound mapping -- bound_codes /
bound_map (hsc_compact_dev.h) with the group tables in LDS and in global
memory, with and without the point index (k_ph_insert / ph_find / ph_key),
code_of (hsc_compact.hip) for keys of more than 8 words, and cnarrow_bound
(hsc_narrow.hip) -- bit for bit against the integer model of
tests/compact_placed.py (pinned to the CPU sort-join and to the rule
restatement by tests/test_compact_placed_model.py).

Every case runs on a context of its own: the rows go in as device rows
(hsc_window_ingest_device), the batches through hsc_probe_device into verdict
bytes of 0xFF and a bitmap of ones.  A read set is one range, its bounds placed
by branch of the mapping rule next to their neighbouring rows, its snapshot the
far row's LSN or the LSN before: a bound that is off by one row, a step that
stops at a code word, a lost spare bit or a point compared with >= fails here.
Every arm asserts the path it means to take and runs the three batch orders
(whole waves of points, points and ranges alternating, shuffled)."""

import functools

import numpy as np
import pytest

import appended_model as A
import compact_placed as P
from comdb2_amd.hsc import (LAYOUT_AUTO, LAYOUT_COMPACT, LAYOUT_COMPACT_WIDE, LAYOUT_NARROW, LAYOUT_WIDE,
                            PATH_NO_COMP_NARROW, PATH_NO_CT_POINTS, Validator)
from test_gpu_appended_placed import probe

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 2048                    # rows of a compact tile
BOUND_LDS = 48 * 1024          # the bound kernel's tables stay in LDS up to this
# windows that would otherwise take the narrow index (over compressed codes)
PATHS = {"w2-63": PATH_NO_COMP_NARROW, "w3-62": PATH_NO_COMP_NARROW}
TILED = [n for n in P.NAMES if P.EXPECT[n][1]]
COMPACT = [n for n in P.NAMES if P.EXPECT[n][0] is not None]


@pytest.fixture
def ctx():
    """ctx(groups, layout, paths) -> a Validator of its own, closed after the test."""
    made = []

    def make(groups, layout=LAYOUT_AUTO, paths=0):
        v = Validator(0)
        made.append(v)
        for g, (tb, ix, klen) in enumerate(groups):
            assert v.register_group(tb, ix, klen) == g
        v.set_layout(layout)
        v.set_paths(paths)
        return v

    yield make
    for v in made:
        v.close()


def ingest(v, rows):
    dev = torch.device("cuda", 0)
    tg = torch.from_numpy(rows.gid.astype(np.int32)).to(dev)
    tw = torch.from_numpy(rows.words.reshape(-1).view(np.int64)).to(dev)
    tl = torch.from_numpy(rows.lsn.view(np.int64)).to(dev)
    v.ingest_device(len(rows), rows.words.shape[0], tg.data_ptr(), tw.data_ptr(), tl.data_ptr(),
                    int(rows.lsn.max()) + 1)
    torch.cuda.synchronize()
    assert v.words == rows.words.shape[0] and v.keys == len(rows)


@functools.lru_cache(maxsize=None)
def wanted(name, order):
    c = P.case(name)
    return c.model().verdicts(c.batch(order))


def same(got, want, what):
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(want)} read sets differ, first {bad[:8].tolist()}: " \
                          f"want {want[bad[:8]].tolist()}"


def records(v, m):
    """(verdicts, join records) of one probe."""
    v.enable_timing(True)
    got = probe(v, m)
    v.synchronize()
    rec = v.timing()["records"]
    v.enable_timing(False)
    return got, rec


def compact_window(v, c, name):
    cw, tkw = P.EXPECT[name]
    assert v.layout == LAYOUT_COMPACT and v.code_words == cw and v.tile_key_words == tkw


def bound_lds_bytes(c):
    ng = len(c.groups)
    return ng * (c.W | 1) * 64 + 8 * ng


@pytest.mark.parametrize("name", TILED)
def test_compact_tiles(ctx, name):
    """Dense batches on the compact tiles: with the point index (a probe whose
    code bounds are equal is answered in the bound kernel) and with
    PATH_NO_CT_POINTS (points take join records)."""
    c = P.case(name)
    if name == "w8-many":      # the tables no longer fit LDS: the kernel reads them in place
        assert c.W == 8 and bound_lds_bytes(c) > BOUND_LDS
    else:
        assert bound_lds_bytes(c) <= BOUND_LDS
    arms = []
    for paths in (0, PATH_NO_CT_POINTS):
        v = ctx(c.groups, LAYOUT_AUTO, PATHS.get(name, 0) | paths)
        ingest(v, c.rows)
        compact_window(v, c, name)
        assert v.words == c.W
        arms.append(v)
    for order in P.ORDERS:
        m = c.batch(order)
        assert m["n"] >= 8 * ((c.n + TILE - 1) // TILE)   # dense: the batch takes the tiles
        got, with_index = records(arms[0], m)
        same(got, wanted(name, order), f"{order}, point index")
        got, without = records(arms[1], m)
        same(got, wanted(name, order), f"{order}, join records")
        if c.W <= 8:
            assert with_index < without, (order, with_index, without)
        else:                   # longer keys have no point index: the generic bound kernel
            assert c.W == 9 and with_index == without


@pytest.mark.parametrize("name", COMPACT)
def test_wide_compact_pipeline(ctx, name):
    """The wide tile pipeline over compact codes: LAYOUT_COMPACT_WIDE on the
    windows that have compact tiles, LAYOUT_AUTO on those whose tile key would
    need a fourth word."""
    c = P.case(name)
    tiled = P.EXPECT[name][1] > 0
    v = ctx(c.groups, LAYOUT_COMPACT_WIDE if tiled else LAYOUT_AUTO, PATHS.get(name, 0))
    ingest(v, c.rows)
    compact_window(v, c, name)
    for order in P.ORDERS:
        same(probe(v, c.batch(order)), wanted(name, order), order)


def test_sparse_batches(ctx):
    """Fewer than 8 probes per tile on a window of compact tiles: the batch
    takes the wide pipeline over compact codes."""
    name = "w3-64"
    c = P.case(name)
    v = ctx(c.groups, LAYOUT_AUTO)
    ingest(v, c.rows)
    compact_window(v, c, name)
    assert c.n <= TILE
    m = c.batch("shuffle")
    got = np.concatenate([probe(v, A.slice_batch(m, a, min(a + 7, m["n"]))) for a in range(0, m["n"], 7)])
    same(got, wanted(name, "shuffle"), "slices of 7")


def test_narrow_compressed_codes(ctx):
    """Varying bits totalling <= 62 over the whole window: by default the
    narrow index over compressed codes answers (cnarrow_bound)."""
    name = "w3-62"
    c = P.case(name)
    v = ctx(c.groups, LAYOUT_AUTO)
    ingest(v, c.rows)
    assert v.layout == LAYOUT_NARROW
    for order in P.ORDERS:
        same(probe(v, c.batch(order)), wanted(name, order), order)


def test_not_compact(ctx):
    """384 varying bits would need a seventh code word: the window stays wide."""
    name = "w8-384"
    c = P.case(name)
    v = ctx(c.groups, LAYOUT_AUTO)
    ingest(v, c.rows)
    assert v.layout == LAYOUT_WIDE and v.code_words == 8 and v.tile_key_words == 0
    for order in P.ORDERS:
        same(probe(v, c.batch(order)), wanted(name, order), order)


def test_rebuilds_reuse_the_point_buffer(ctx):
    """Two windows of equal size and disjoint keys, one after the other and
    the first again in one context: the point index is rebuilt in place at
    epochs 1, 2 and 3; points on the other window's rows miss, on its own hit."""
    c = P.rebuild_case()
    v = ctx(c.GROUPS, LAYOUT_AUTO)
    for w in (0, 1, 0):
        ingest(v, c.rows(w))
        assert v.layout == LAYOUT_COMPACT
        assert v.code_words == c.code_words and v.tile_key_words == c.tile_key_words
        m = c.batch(w)
        same(probe(v, m), P.Model(c.W, c.rows(w)).verdicts(m), f"window {w}")


@pytest.mark.parametrize("arm", ["point-index", "join-records", "wide"])
def test_snapshot_clamps(ctx, arm):
    """Points and ranges on the oldest, the newest and another row with the
    snapshot at the row's LSN, the LSN before, 0, below the oldest commit and
    above the newest (by 1, by 2^32 and at 2^62)."""
    name = "w3-64"
    c = P.case(name)
    v = ctx(c.groups, LAYOUT_COMPACT_WIDE if arm == "wide" else LAYOUT_AUTO,
            PATH_NO_CT_POINTS if arm == "join-records" else 0)
    ingest(v, c.rows)
    compact_window(v, c, name)
    m = c.snapshot_batch()
    assert m["n"] >= 8
    want = c.model().verdicts(m)
    assert 0 < want.sum() < len(want)
    same(probe(v, m), want, arm)
