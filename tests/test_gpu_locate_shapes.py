"""GPU parity of the narrow locate's instances (k_locate_t,
comdb2_amd/csrc/hsc_narrow.hip): the fast ones, built for a window of 1 or 2
key words whose last word varies, with the bucket table, no compressed codes
and 32-bit commit ranks, and the general one every other window takes.
hsc_batch_stats tells which ran (fast_locates / general_locates).

As in test_gpu_locate_staging.py a window is a few 4096-row tiles (full ones
and a partial last one) ingested as device rows on the 8-byte-row tile
pipeline (LAYOUT_NARROW_TILES).  One range per read set, in batch order (probe
i = read set i, asserted), so every range's verdict is compared and a range's
place in the batch fixes its lane (i % 64), its sub-chunk (i // 1024 % 4) and
its chunk (i // 4096).  Expected verdicts are the CPU sort-join's
(oracle/sortjoin.c) over the same rows and the same marshalled probes.

A fast instance maps a wave's bounds by the short form (hsc_reldiff.h) when
every lane's gid is the window's and, for 2 words, word 0 of both bounds is
at or above the base's by less than 2^tz; otherwise the whole wave takes the
full form.  For the 9-byte int64 keys (tz = 56) a bound qualifies when its
value is >= KEY0 rounded down to 256; a range of a second registered group
(no rows) never does.
"""

import numpy as np
import pytest

from comdb2_amd import formats as F
from comdb2_amd import hsc
from comdb2_amd.formats import Range, ReadSets
from comdb2_amd.hsc import LAYOUT_NARROW, LAYOUT_NARROW_TILES, PATH_TILE_DIR, Validator
from comdb2_amd.workloads import int64_words

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 4096
PARTIAL = 777            # rows of the last tile
KEY0, KEY_STEP = 1000, 7
QUAL_FROM = KEY0 & ~255  # int64 keys: bounds from here up share word 0's range with the base
LSN0 = (5 << 32) + 4096
CHUNK, SUB = 4096, 1024
NB = CHUNK + SUB + 37    # a batch: two chunks, the second one ending in a partial wave


class Win:
    """Rows (gid, words[W], lsn) sorted by (gid, key), and per group: table
    name, key length, the rows' key values and how a value becomes the bytes
    of a lower / upper bound."""

    def __init__(self, groups, gid, vals, words, lsn):
        self.groups = groups            # [(table, keylen, enc_lo, enc_hi)]
        self.gid, self.vals, self.words, self.lsn = gid, vals, words, lsn
        self.ntiles = (len(gid) + TILE - 1) // TILE

    def of(self, g):
        sel = self.gid == g
        return self.vals[sel], self.lsn[sel]


def lsns(n, mod=1 << 20, mul=2654435761):
    i = np.arange(n, dtype=np.uint64)
    return np.uint64(LSN0) + (i * np.uint64(mul) + (i >> np.uint64(12)) * np.uint64(40503)) % np.uint64(mod)


def nrows(ntiles):
    return (ntiles - 1) * TILE + PARTIAL


def be_words(rows):
    """uint8[n, 8 W] big-endian key bytes -> uint64[W][n]"""
    n = rows.shape[0]
    return rows.view(">u8").astype(np.uint64).reshape(n, -1).T.copy()


def win_int64(ntiles=3, lsn_mod=1 << 20, vals=None):
    """9-byte int64 keys: W = 2, lw = 2, tz = 56."""
    if vals is None:
        vals = KEY0 + KEY_STEP * np.arange(nrows(ntiles), dtype=np.int64)
    n = len(vals)
    return Win([("t1", 9, F.enc_int64, F.enc_int64), ("t2", 9, F.enc_int64, F.enc_int64)],
               np.zeros(n, np.uint32), vals, int64_words(vals), lsns(n, lsn_mod))


def be8(v):
    return int(v).to_bytes(8, "big")


def win_u64(ntiles=3):
    """8-byte big-endian keys: W = 1, lw = 1, tz = 0 (odd step)."""
    vals = KEY0 + KEY_STEP * np.arange(nrows(ntiles), dtype=np.int64)
    n = len(vals)
    return Win([("t1", 8, be8, be8), ("t2", 8, be8, be8)], np.zeros(n, np.uint32), vals,
               vals.astype(np.uint64).reshape(1, n).copy(), lsns(n))


TAIL = bytes([0x42, 1, 2, 3, 4, 5, 6, 7])


def win_last_word_constant(ntiles=3):
    """16-byte keys whose last word never varies: W = 2, lw = 1.  A lower
    bound ends in zeros and an upper one in 0xFF, so the words below lw decide
    nothing but are there."""
    vals = KEY0 + KEY_STEP * np.arange(nrows(ntiles), dtype=np.int64)
    n = len(vals)
    words = np.stack([vals.astype(np.uint64), np.full(n, int.from_bytes(TAIL, "big"), np.uint64)])
    return Win([("t1", 16, lambda v: be8(v) + bytes(8), lambda v: be8(v) + b"\xff" * 8)],
               np.zeros(n, np.uint32), vals, words, lsns(n))


def win_two_groups(ntiles=5):
    """Rows of two groups (gid 0 and 1), 20-odd varying bits each: too far
    apart for one 62-bit span, few enough for compressed codes.  Five tiles,
    so that group 0 holds two whole tiles (whole_tiles)."""
    n = nrows(ntiles)
    n0 = n // 2
    vals = np.concatenate([KEY0 + KEY_STEP * np.arange(n0, dtype=np.int64),
                           KEY0 + 5 * np.arange(n - n0, dtype=np.int64)])
    gid = np.concatenate([np.zeros(n0, np.uint32), np.ones(n - n0, np.uint32)])
    return Win([("t1", 9, F.enc_int64, F.enc_int64), ("t2", 9, F.enc_int64, F.enc_int64)], gid, vals,
               int64_words(vals), lsns(n))


def win_three_words(ntiles=3):
    """18-byte keys enc(7) || enc(v): W = 3."""
    vals = KEY0 + KEY_STEP * np.arange(nrows(ntiles), dtype=np.int64)
    n = len(vals)
    rows = np.zeros((n, 24), np.uint8)
    rows[:, :9] = F.enc_int64_array(np.full(n, 7, np.int64))
    rows[:, 9:18] = F.enc_int64_array(vals)
    enc = lambda v: F.enc_int64(7) + F.enc_int64(v)
    return Win([("t1", 18, enc, enc)], np.zeros(n, np.uint32), vals, be_words(rows), lsns(n))


def win_skewed(ntiles=40, sparse=8):
    """Dense keys, then `sparse` tiles of keys 2^20 apart: the tiles' first
    codes crowd the linear table's first bucket, so the build takes log mode."""
    n = nrows(ntiles)
    nd = (ntiles - sparse) * TILE
    vals = np.concatenate([KEY0 + np.arange(nd, dtype=np.int64),
                           KEY0 + nd + (np.arange(1, n - nd + 1, dtype=np.int64) << 20)])
    return win_int64(vals=vals)


# ---- ranges --------------------------------------------------------------------
def random_ranges(w, n, rng, g=0):
    """(g, lo, hi) around rows picked by index: narrow, all within the window's
    first and last key (so they qualify for the short form)."""
    vals, _ = w.of(g)
    r = rng.integers(0, len(vals), n)
    e = np.minimum(len(vals) - 1, r + rng.integers(0, 40, n))
    return [(g, int(vals[a]) - int(rng.integers(0, 2)), int(vals[b]) + int(rng.integers(0, 2)))
            for a, b in zip(r, e)]


def placed_ranges(w, g=0):
    """The ranges the module docstring of test_gpu_locate_staging.py lists for
    a tile's first key, at every tile, and the window's ends; point ranges,
    the whole window, bounds below and above it and past saturation."""
    vals, _ = w.of(g)
    first, last = int(vals[0]), int(vals[-1])
    out = []
    edges = [int(vals[t * TILE]) for t in range((len(vals) + TILE - 1) // TILE)] + [last]
    for f in edges:
        for e in (f - 1, f, f + 1):
            for d in (0, 1, KEY_STEP, 40 * KEY_STEP):
                out.append((g, e - d, e))
                out.append((g, e, e + d))
    for k in (first, last, int(vals[len(vals) // 2]), int(vals[5]) + 1):  # points (the last: no row)
        out.append((g, k, k))
    out += [(g, first, last), (g, first - 1, last + 1), (g, first - 50, last + 5000)]  # the whole window
    out += [(g, max(0, first - 900), first - 1), (g, 0, max(0, first - 300)), (g, 0, first + 3),
            (g, 0, 5)]  # below it (0: below QUAL_FROM as well)
    out += [(g, last + 1, last + 10_000), (g, last - 3, last + 10_000)]  # above it
    sat = (1 << 62) + 12345
    out += [(g, first + 10, first + sat), (g, first + sat, first + sat + 5), (g, 0, first + sat),
            (g, last, (1 << 63) - 1)]  # past saturation
    return out


def reversed_ranges(w, g=0):
    """lo > hi.  The host's marshal drops such a range (its read set keeps
    verdict 0), so they go at the end of a batch, where they shift no probe;
    run() also swaps the marshalled bounds of a few probes, which reach the
    kernel reversed."""
    vals, _ = w.of(g)
    first, last = int(vals[0]), int(vals[-1])
    return [(g, first + 500, first + 400), (g, last, first), (g, first + 1, first)]


SWAPPED = (2040, 2041, 2042, 2043)  # probes whose bounds run() swaps


def whole_tiles(w, g=0):
    """Ranges that cover whole tiles: all of tile 1; tiles 0 and 1; a part of
    tile 0, all of tile 1, a part of tile 2."""
    vals, _ = w.of(g)
    f = lambda t: int(vals[t * TILE])
    return [(g, f(1), f(2) - 1), (g, f(0) - 1, f(2) - 1), (g, f(0) + 100, f(2) + 100)]


def snapshots(w, ranges, rng):
    """Per range: the newest commit among its rows (no conflict) or the LSN
    before (a conflict), half each; a range without rows: the middle of the span."""
    mid = int(w.lsn.min()) + (int(w.lsn.max()) - int(w.lsn.min())) // 2
    snaps = np.full(len(ranges), mid, np.uint64)
    for g in range(len(w.groups)):
        vals, lsn = w.of(g)
        idx = [i for i, r in enumerate(ranges) if r[0] == g]
        if not idx or not len(vals):
            continue
        b = np.array([[ranges[i][1], ranges[i][2]] for i in idx], dtype=object)
        pa = np.searchsorted(vals, np.array([min(int(x), (1 << 63) - 1) for x in b[:, 0]], np.int64), "left")
        pb = np.searchsorted(vals, np.array([min(int(x), (1 << 63) - 1) for x in b[:, 1]], np.int64), "right")
        for k, i in enumerate(idx):
            if pa[k] < pb[k]:
                snaps[i] = int(lsn[pa[k]:pb[k]].max()) - int(rng.integers(0, 2))
    return snaps


def readsets(w, ranges, snaps):
    sets = []
    for g, lo, hi in ranges:
        tb, _, enc_lo, enc_hi = w.groups[g]
        sets.append([Range(tb, 0, enc_lo(lo), enc_hi(hi))])
    return ReadSets.from_lists(sets, [int(s) for s in snaps], tbnames=[x[0] for x in w.groups])


def qualifies(ranges):
    """int64 keys, W = 2: which probes meet the short form's precondition."""
    return np.array([g == 0 and lo >= QUAL_FROM and hi >= QUAL_FROM for g, lo, hi in ranges])


# ---- device side -------------------------------------------------------------------
@pytest.fixture
def make_validator():
    made = []

    def make(w):
        v = Validator(0)
        made.append(v)
        for g, (tb, keylen, _, _) in enumerate(w.groups):
            assert v.register_group(tb, 0, keylen) == g
        v.set_layout(LAYOUT_NARROW_TILES)
        return v
    yield make
    for v in made:
        v.close()


def ingest(v, w):
    dev = torch.device("cuda", 0)
    tg = torch.from_numpy(w.gid.astype(np.int32)).to(dev)
    tw = torch.from_numpy(np.ascontiguousarray(w.words).reshape(-1).view(np.int64)).to(dev)
    tl = torch.from_numpy(w.lsn.view(np.int64)).to(dev)
    v.ingest_device(len(w.gid), w.words.shape[0], tg.data_ptr(), tw.data_ptr(), tl.data_ptr(),
                    int(w.lsn.max()) + 1)
    torch.cuda.synchronize()
    assert v.layout == LAYOUT_NARROW


def probe(v, m, bitmap=False):
    """The marshalled batch through hsc_probe_device; verdict bytes prefilled
    with 0xFF (and the bitmap with ones): the batch must write all of them."""
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    u = {k: t(m[k]) for k in ("lo", "hi", "gid", "snap", "txn", "lock_table", "lock_snap", "lock_txn")}
    T = m["n_txn"]
    verdict = torch.full((max(T, 1),), 0xFF, dtype=torch.uint8, device=dev)
    bits = torch.full(((T + 63) // 64,), -1, dtype=torch.int64, device=dev) if bitmap else None
    torch.cuda.synchronize()
    v.probe_device(hsc.ProbeBatch(m["n"], u["lo"].data_ptr(), u["hi"].data_ptr(), u["gid"].data_ptr(),
                                  u["snap"].data_ptr(), u["txn"].data_ptr(), m["n_lock"],
                                  u["lock_table"].data_ptr(), u["lock_snap"].data_ptr(),
                                  u["lock_txn"].data_ptr(), T, verdict.data_ptr(),
                                  bits.data_ptr() if bitmap else 0))
    torch.cuda.synchronize()
    got = verdict.cpu().numpy()[:T]
    assert set(np.unique(got)) <= {0, 1}
    if bitmap:
        b = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")
        np.testing.assert_array_equal(b[:T].astype(bool), got != 0)
        assert not b[T:].any()
    return got != 0


def reference(w, oracle_mod, m, table_max):
    sj = oracle_mod.SortJoin(w.gid, w.words, w.lsn, len(w.groups))
    want, _ = sj.probe(m, table_max, nthreads=8)
    sj.close()
    return want != 0


def counters(v):
    s = v.batch_stats()
    return np.array([s["fast_locates"], s["general_locates"], s["column_batches"] + s["plan_batches"]])


def run(v, w, oracle_mod, ranges, seed, expect, bitmap=False):
    """Probe `ranges` (one per read set) followed by reversed_ranges, and
    compare with the sort-join; expect = the rise of (fast_locates,
    general_locates, dense batches)."""
    ranges = ranges + reversed_ranges(w)
    snaps = snapshots(w, ranges, np.random.default_rng(seed))
    m = v.marshal(readsets(w, ranges, snaps))
    assert m["n"] == len(ranges) - 3 and m["n_lock"] == 0 and m["n_txn"] == len(ranges)
    np.testing.assert_array_equal(m["txn"], np.arange(m["n"]))  # probe i = read set i
    for i in SWAPPED:
        lo = m["lo"][:, i].copy()
        m["lo"][:, i] = m["hi"][:, i]
        m["hi"][:, i] = lo
    want = reference(w, oracle_mod, m, v.table_max())
    before = counters(v)
    got = probe(v, m, bitmap)
    np.testing.assert_array_equal(counters(v) - before, expect)
    np.testing.assert_array_equal(got, want)
    return want


FAST, GENERAL = (1, 0, 1), (0, 1, 1)


def placed_batch(w, rng, nq=None):
    """NB ranges: random qualifying ones, the placed ones from index 2048 on,
    whole-tile ranges in the first chunk's first and last sub-chunk and in
    the second chunk."""
    ranges = random_ranges(w, NB, rng)
    special = placed_ranges(w)
    assert 2048 + len(special) < 3 * SUB
    ranges[2048:2048 + len(special)] = special
    wt = whole_tiles(w)
    for base in (10, 3 * SUB + 10, CHUNK + 10):  # sub-chunk 0, the last sub-chunk, the next chunk
        ranges[base:base + len(wt)] = wt
    return ranges


@pytest.mark.parametrize("make_win", [win_int64, win_u64], ids=["w2-int64", "w1-8byte"])
def test_fast_instances_placed_ranges(make_validator, oracle_mod, make_win):
    w = make_win()
    v = make_validator(w)
    ingest(v, w)
    ranges = placed_batch(w, np.random.default_rng(11))
    want = run(v, w, oracle_mod, ranges, 12, FAST)
    assert 0 < int(want.sum()) < len(want)
    # the whole-tile ranges conflict or not by their snapshot alone: both occur
    idx = [b + k for b in (10, 3 * SUB + 10, CHUNK + 10) for k in range(3)]
    assert 0 < int(want[idx].sum()) < len(idx)


def other_group(w, rng, n):
    """Ranges of the second registered group, which has no rows: their gid is
    not the window's."""
    vals, _ = w.of(0)
    return [(1, int(a), int(a) + 50) for a in rng.choice(vals, n)]


def high_word_differs(w, rng, n):
    """int64 ranges that start below QUAL_FROM (word 0 below the base's) and
    end inside the window: not qualifying, and with rows."""
    vals, _ = w.of(0)
    return [(0, int(rng.integers(0, QUAL_FROM)), int(vals[int(rng.integers(0, 3 * TILE // 2))]))
            for _ in range(n)]


@pytest.mark.parametrize("make_win,kinds", [(win_int64, (other_group, high_word_differs)),
                                            (win_u64, (other_group,))], ids=["w2-int64", "w1-8byte"])
def test_wave_mixing(make_validator, oracle_mod, make_win, kinds):
    w = make_win()
    v = make_validator(w)
    ingest(v, w)
    rng = np.random.default_rng(21)
    ranges = random_ranges(w, NB, rng)
    # wave 0 all qualifying; one non-qualifying probe at lane 0 (wave 1), lane
    # 63 (wave 2), lane 31 (wave 3); every second lane (wave 4); a whole wave
    # (wave 5); either side of a sub-chunk and of a chunk boundary; the last
    # probe, in the partial wave
    spots = [64, 2 * 64 + 63, 3 * 64 + 31] + list(range(4 * 64, 5 * 64, 2)) + list(range(5 * 64, 6 * 64))
    # (1023 alone, 1024 qualifying; 2047 qualifying, 2048 alone; 3071 and 3072
    # both; 4095 and 4096 both, the last and the first probe of a chunk)
    spots += [SUB - 1, 2 * SUB, 3 * SUB - 1, 3 * SUB, CHUNK - 1, CHUNK, NB - 1]
    for k, i in enumerate(spots):
        ranges[i] = kinds[k % len(kinds)](w, rng, 1)[0]
    nq = np.zeros(NB, bool)
    nq[spots] = True
    if make_win is win_int64:
        np.testing.assert_array_equal(~qualifies(ranges), nq)
    waves = nq[: NB // 64 * 64].reshape(-1, 64)
    assert not waves[0].any() and waves[5].all() and waves[4].sum() == 32
    assert [int(x.sum()) for x in waves[1:4]] == [1, 1, 1]
    assert nq[SUB - 1] and not nq[SUB] and nq[CHUNK - 1] and nq[CHUNK] and NB % 64 != 0
    want = run(v, w, oracle_mod, ranges, 22, FAST)
    assert 0 < int(want.sum()) < len(want)
    if make_win is win_int64:  # the non-qualifying probes with rows conflict or not, too
        assert 0 < int(want[:NB][nq].sum()) < int(nq.sum())


GENERAL_WINDOWS = {
    "lw-below-W": (win_last_word_constant, 0),
    "compressed-two-groups": (win_two_groups, 0),
    "three-words": (win_three_words, 0),
    "tile-directory": (win_int64, PATH_TILE_DIR),
    "commit-directory": (lambda: win_int64(lsn_mod=1 << 40), 0),
}


@pytest.mark.parametrize("name", list(GENERAL_WINDOWS))
def test_general_instance(make_validator, oracle_mod, name):
    make_win, paths = GENERAL_WINDOWS[name]
    w = make_win()
    if name == "commit-directory":
        assert int(w.lsn.max()) - int(w.lsn.min()) >= 1 << 32
    v = make_validator(w)
    v.set_paths(paths)
    ingest(v, w)
    rng = np.random.default_rng(31)
    ranges = random_ranges(w, 2500, rng)
    special = placed_ranges(w)
    ranges[100:100 + len(special)] = special
    wt = whole_tiles(w)
    ranges[10:10 + len(wt)] = wt
    if name == "compressed-two-groups":
        g1 = random_ranges(w, 600, rng, g=1) + placed_ranges(w, g=1)
        ranges[1200:1200 + len(g1)] = g1
    want = run(v, w, oracle_mod, ranges, 32, GENERAL)
    assert 0 < int(want.sum()) < len(want)


def test_log_table_fast_instance(make_validator, oracle_mod):
    w = win_skewed()
    v = make_validator(w)
    ingest(v, w)
    rng = np.random.default_rng(41)
    ranges = random_ranges(w, 3000, rng)
    special = placed_ranges(w)
    ranges[100:100 + len(special)] = special
    wt = whole_tiles(w)
    ranges[10:10 + len(wt)] = wt
    ranges[2000:2010] = high_word_differs(w, rng, 10)
    before = v.batch_stats()["plan_batches"]
    want = run(v, w, oracle_mod, ranges, 42, FAST)
    assert v.batch_stats()["plan_batches"] == before + 1  # log mode: the batch took the plan path
    assert 0 < int(want.sum()) < len(want)


def test_small_batches(make_validator, oracle_mod):
    w = win_int64()
    v = make_validator(w)
    ingest(v, w)
    # table locks only: no probe arrays, so the general instance (or none)
    # (snapshots: the oldest commit and the newest one alternate)
    snaps = [LSN0 if i % 2 else int(w.lsn.max()) for i in range(2500)]
    rs = ReadSets.from_lists([[Range.locked("t1")] for _ in range(2500)], snaps, tbnames=["t1", "t2"])
    m = v.marshal(rs)
    assert m["n"] == 0 and m["n_lock"] == 2500
    want = reference(w, oracle_mod, m, v.table_max())
    before = counters(v)
    got = probe(v, m)
    rise = counters(v) - before
    assert rise[0] == 0 and rise[2] == 0
    np.testing.assert_array_equal(got, want)
    # an empty batch: read sets without ranges
    rs = ReadSets.from_lists([[] for _ in range(2500)], [LSN0] * 2500, tbnames=["t1", "t2"])
    m = v.marshal(rs)
    assert m["n"] == 0 and m["n_lock"] == 0 and m["n_txn"] == 2500
    before = counters(v)
    got = probe(v, m)
    np.testing.assert_array_equal(counters(v) - before, (0, 0, 0))
    assert not got.any()
    # a batch that asks for the bitmap
    ranges = placed_batch(w, np.random.default_rng(51))
    want = run(v, w, oracle_mod, ranges, 52, FAST, bitmap=True)
    assert 0 < int(want.sum()) < len(want)


def test_rebuild_between_shapes(make_validator, oracle_mod):
    """The same context from a fast-shape window to a general-shape one (its
    commits span 2^32 and more) and back: the instance follows the window."""
    fast, general = win_int64(), win_int64(lsn_mod=1 << 40)
    v = make_validator(fast)
    rng = np.random.default_rng(61)
    for k, (w, expect) in enumerate([(fast, FAST), (general, GENERAL), (fast, FAST)]):
        ingest(v, w)
        ranges = random_ranges(w, 2500, rng)
        wt = whole_tiles(w)
        ranges[10:10 + len(wt)] = wt
        want = run(v, w, oracle_mod, ranges, 62 + k, expect)
        assert 0 < int(want.sum()) < len(want)
    s = v.batch_stats()
    assert (s["fast_locates"], s["general_locates"]) == (2, 1)
