"""GPU parity of the narrow tile join that scans its own column
(k_join_t<true>, comdb2_amd/csrc/hsc_narrow.hip): on a balanced window no plan
kernel runs -- a join block loads its tile's entries of the locate's
chunk-major table, scans them over its 8 waves, runs every record of the tile
in rounds of 1024 and moves its share of the locate's flags into the caller's
verdict bytes, which the locate has cleared.

Every window is one index of distinct int64 keys KEY0 + KEY_STEP i ingested as
device rows (hsc_window_ingest_device, LAYOUT_NARROW_TILES): ntiles - 1 full
4096-row tiles and a partial last one; the commit LSNs span < 2^32.  Batches
are built as probe columns (one range or one table lock per read set), probed
with hsc_probe_device into verdict bytes prefilled with 0xFF, and compared with
the CPU sort-join (oracle/sortjoin.c) over the same rows and columns.  A range
drawn inside a tile gives that tile exactly one join record, so the batches
place their records: G = ceil(ranges / 4096) chunks, records per tile, tiles
and chunk runs left empty.  Every case runs on a context of its own (the path
of a batch depends on the context's last 64 batches) and checks through
hsc_batch_stats which path its batches took.
"""

import numpy as np
import pytest

from comdb2_amd import hsc
from comdb2_amd.hsc import LAYOUT_NARROW, LAYOUT_NARROW_TILES, Validator
from comdb2_amd.workloads import int64_words

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 4096            # rows per tile
CHUNK = 4096           # probes per locate workgroup (a column entry of the join)
TILE_CAP = 1024        # records a join block runs per round
HOT_BATCHES = 64       # batches that take the plan path after one with a tile past TILE_CAP
KEY0, KEY_STEP = 1000, 7
LSN0 = (5 << 32) + 4096  # oldest commit; the span stays below 2^32
LSN_MOD = 1 << 20
PARTIAL = 777          # rows of the last tile
NEVER = 1 << 62        # a snapshot after every commit


class Window:
    """Rows of a window of `ntiles` tiles, their sort-join and range maxima."""

    def __init__(self, ntiles):
        self.ntiles = ntiles
        n = (ntiles - 1) * TILE + PARTIAL
        i = np.arange(n, dtype=np.uint64)
        self.keys = (KEY0 + KEY_STEP * i).astype(np.int64)
        # a fixed scramble of the row index: every tile holds old and new rows
        self.lsn = np.uint64(LSN0) + (i * np.uint64(2654435761) + (i >> np.uint64(12)) * np.uint64(40503)) % np.uint64(LSN_MOD)
        self.words = int64_words(self.keys)
        self.sj = None
        self._levels = [self.lsn]

    def first(self, t):
        return int(self.keys[t * TILE])

    def rows_of(self, t):
        return np.minimum(TILE, len(self.keys) - np.asarray(t, dtype=np.int64) * TILE)

    def range_max(self, pa, pb):
        """max lsn[pa:pb) per pair (pb > pa), by a sparse table grown on demand."""
        ln = pb - pa
        lv = np.floor(np.log2(ln)).astype(np.int64)
        while len(self._levels) <= int(lv.max()):
            m, h = self._levels[-1], 1 << (len(self._levels) - 1)
            self._levels.append(np.maximum(m[:-h], m[h:]))
        out = np.empty(len(pa), dtype=np.uint64)
        for l in np.unique(lv):
            s = lv == l
            m = self._levels[l]
            out[s] = np.maximum(m[pa[s]], m[pb[s] - (1 << int(l))])
        return out

    def sortjoin(self, oracle_mod):
        if self.sj is None:
            self.sj = oracle_mod.SortJoin(np.zeros(len(self.lsn), np.uint32), self.words, self.lsn, 1)
        return self.sj


_windows = {}


def window(ntiles):
    if ntiles not in _windows:
        _windows[ntiles] = Window(ntiles)
    return _windows[ntiles]


@pytest.fixture(scope="module", autouse=True)
def _close_windows():
    yield
    for w in _windows.values():
        if w.sj is not None:
            w.sj.close()
    _windows.clear()


def narrow_ranges(w, tiles, seed, conflicts="half", empties=True):
    """One range inside each tile of `tiles` (int array): rows r0 .. r0 + k of
    the tile, 1 <= r0, k < 40, the bounds up to 3 off the end rows' keys (keys
    are KEY_STEP apart), or with `empties` between two keys (no row) for one
    range in ten.  The snapshot is the newest commit among the range's rows
    (no conflict) or the LSN before it (a conflict): "half" of each, "all"
    conflicts or "none" (a snapshot after every commit).  Returns (lo, hi, snap)."""
    rng = np.random.default_rng(seed)
    tiles = np.asarray(tiles, dtype=np.int64)
    n = len(tiles)
    rows = w.rows_of(tiles)
    k = rng.integers(0, 40, n)
    r0 = 1 + (rng.integers(0, 1 << 30, n) % (rows - 2 - k))
    pa = tiles * TILE + r0
    pb = pa + k + 1
    lo = w.keys[pa] - rng.integers(0, 4, n)
    hi = w.keys[pb - 1] + rng.integers(0, 4, n)
    empty = (rng.integers(0, 10, n) == 0) & empties
    lo[empty] = w.keys[pa[empty]] + 1
    hi[empty] = w.keys[pa[empty]] + 5
    coin = rng.integers(0, 2, n).astype(np.uint64)
    snap = w.range_max(pa, pb) - (coin if conflicts == "half" else np.uint64(1))
    snap[empty] = LSN0 + LSN_MOD // 2
    if conflicts == "none":
        snap[:] = NEVER
    return lo, hi, snap


def batch(lo, hi, snap, txn, n_txn, lock_snap=(), lock_txn=()):
    """Probe columns in the marshalled layout (Validator.marshal)."""
    z32 = np.zeros(0, np.uint32)
    return dict(words=2, n=len(lo), n_lock=len(lock_snap), n_txn=n_txn,
                lo=int64_words(np.asarray(lo, np.int64)) if len(lo) else np.zeros((2, 0), np.uint64),
                hi=int64_words(np.asarray(hi, np.int64)) if len(hi) else np.zeros((2, 0), np.uint64),
                gid=np.zeros(len(lo), np.uint32), snap=np.asarray(snap, np.uint64),
                txn=np.asarray(txn, np.uint32),
                lock_table=np.zeros(len(lock_snap), np.uint32) if len(lock_snap) else z32,
                lock_snap=np.asarray(lock_snap, np.uint64), lock_txn=np.asarray(lock_txn, np.uint32),
                forced=np.zeros(n_txn, np.uint8))


def placed_batch(w, tiles, seed, conflicts="half"):
    """One single-range read set per entry of `tiles`."""
    lo, hi, snap = narrow_ranges(w, tiles, seed, conflicts)
    return batch(lo, hi, snap, np.arange(len(tiles)), len(tiles))


def reference(w, oracle_mod, m, table_max):
    want, _ = w.sortjoin(oracle_mod).probe(m, table_max, nthreads=8)
    return want != 0


# ---- device side -----------------------------------------------------------
@pytest.fixture
def fresh():
    v = Validator(0)
    assert v.register_group("t1", 0, 9) == 0
    v.set_layout(LAYOUT_NARROW_TILES)
    yield v
    v.close()


def ingest(v, w):
    dev = torch.device("cuda", 0)
    tg = torch.zeros(len(w.keys), dtype=torch.int32, device=dev)
    tw = torch.from_numpy(w.words.reshape(-1).view(np.int64)).to(dev)
    tl = torch.from_numpy(w.lsn.view(np.int64)).to(dev)
    v.ingest_device(len(w.keys), w.words.shape[0], tg.data_ptr(), tw.data_ptr(), tl.data_ptr(),
                    int(w.lsn.max()) + 1)
    torch.cuda.synchronize()
    assert v.layout == LAYOUT_NARROW
    return v.table_max()


def upload(m):
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {k: t(m[k]) for k in ("lo", "hi", "gid", "snap", "txn", "lock_table", "lock_snap", "lock_txn")}


def outputs(m, bitmap=True):
    """Verdict bytes prefilled with 0xFF and a bitmap of all ones (or None).
    They are filled on torch's stream: synchronise before a probe uses them."""
    dev = torch.device("cuda", 0)
    T = m["n_txn"]
    verdict = torch.full((max(T, 1),), 0xFF, dtype=torch.uint8, device=dev)
    bits = torch.full(((T + 63) // 64,), -1, dtype=torch.int64, device=dev) if bitmap else None
    return verdict, bits


def launch(v, m, u, out):
    """Probe into `out` on the context's current stream (not synchronised)."""
    verdict, bits = out
    T, bitmap = m["n_txn"], bits is not None
    v.probe_device(hsc.ProbeBatch(m["n"], u["lo"].data_ptr(), u["hi"].data_ptr(), u["gid"].data_ptr(),
                                  u["snap"].data_ptr(), u["txn"].data_ptr(), m["n_lock"],
                                  u["lock_table"].data_ptr(), u["lock_snap"].data_ptr(),
                                  u["lock_txn"].data_ptr(), T, verdict.data_ptr(),
                                  bits.data_ptr() if bitmap else 0))
    return out


def result(m, verdict, bits):
    """Verdict bytes (each 0 or 1) as bools; the bitmap must equal them."""
    T = m["n_txn"]
    got = verdict.cpu().numpy()[:T]
    assert set(np.unique(got)) <= {0, 1}
    if bits is not None:
        b = np.unpackbits(bits.cpu().numpy().view(np.uint8), bitorder="little")
        np.testing.assert_array_equal(b[:T].astype(bool), got != 0)
        assert not b[T:].any()
    return got != 0


def probe(v, m, bitmap=True):
    u, out = upload(m), outputs(m, bitmap)
    torch.cuda.synchronize()
    launch(v, m, u, out)
    torch.cuda.synchronize()
    return result(m, *out)


def paths(v):
    s = v.batch_stats()
    return s["column_batches"], s["plan_batches"]


# ---- chunks and tiles --------------------------------------------------------
def round_robin(n, ntiles):
    return np.arange(n) % ntiles


def with_gaps(n, ntiles):
    """Tile 1 gets no record at all; chunk g sends nothing to the tiles t with
    (t + g) % 3 == 0, so a tile's column has empty runs between non-empty ones."""
    g = np.arange(n) // CHUNK
    t = np.arange(n) % ntiles
    bad = (t == 1) | ((t + g) % 3 == 0)
    # move a skipped probe to the next tile this chunk may use
    for _ in range(3):
        t = np.where(bad, (t + 1) % ntiles, t)
        bad = (t == 1) | ((t + g) % 3 == 0)
    assert not bad.any()
    return t


# (ntiles, ranges, placement): G = ceil(ranges / 4096) chunks; every tile of the
# balanced cases holds at most 1024 records
SHAPES = {
    "1tile-g1": (1, 1000, round_robin),
    "3tiles-g1": (3, 3000, round_robin),            # row stride padded 3 -> 4
    "5tiles-g1": (5, CHUNK - 5, round_robin),       # 8 join blocks, 3 past the tiles
    "9tiles-g2": (9, 2 * CHUNK - 5, round_robin),   # 16 join blocks, 7 past the tiles
    "33tiles-g8": (33, 8 * CHUNK - 5, round_robin),  # a chunk row spans two cache lines; hist_stride(8) = 8
    "40tiles-g9": (40, 9 * CHUNK - 5, round_robin),  # hist_stride(9) = 16
    "60tiles-g6-gaps": (60, 6 * CHUNK - 100, with_gaps),
    "300tiles-g64": (300, 64 * CHUNK - 5, round_robin),  # the scan's first wave exactly full
    "300tiles-g65": (300, 65 * CHUNK - 5, round_robin),  # one entry in the second wave
    # kMaxChunks and one below: 2.1 M ranges over 3 tiles, each block ~683 rounds
    "3tiles-g511": (3, 511 * CHUNK - 5, round_robin),
    "3tiles-g512": (3, 512 * CHUNK, round_robin),
}


def shape_batch(name):
    ntiles, n, place = SHAPES[name]
    w = window(ntiles)
    tiles = place(n, ntiles)
    return w, tiles, placed_batch(w, tiles, seed=len(name) + n)


@pytest.mark.parametrize("name", list(SHAPES))
def test_chunks_and_tiles(fresh, oracle_mod, name):
    w, tiles, m = shape_batch(name)
    per_tile = np.bincount(tiles, minlength=w.ntiles)
    hot = int(per_tile.max()) > TILE_CAP
    assert hot == name.startswith("3tiles-g51")
    if "gaps" in name:
        assert per_tile[1] == 0 and per_tile.max() <= TILE_CAP
    tm = ingest(fresh, w)
    want = reference(w, oracle_mod, m, tm)
    assert 0 < int(want.sum()) < len(want)
    got = probe(fresh, m)
    assert paths(fresh) == (1, 0)
    np.testing.assert_array_equal(got, want)


# ---- tile totals around the round size ---------------------------------------
def one_tile_total(w, total, others=500, tile=2):
    """`total` records in one tile, `others` in each of the rest, interleaved."""
    rng = np.random.default_rng(total)
    tiles = np.concatenate([np.full(total, tile)] +
                           [np.full(others, t) for t in range(w.ntiles) if t != tile])
    return rng.permutation(tiles)


@pytest.mark.parametrize("total", [1023, 1024, 1025, 2048, 2049])
def test_tile_totals(fresh, oracle_mod, total):
    w = window(5)
    m = placed_batch(w, one_tile_total(w, total), seed=total)
    tm = ingest(fresh, w)
    want = reference(w, oracle_mod, m, tm)
    assert 0 < int(want.sum()) < len(want)
    np.testing.assert_array_equal(probe(fresh, m), want)
    assert paths(fresh) == (1, 0)
    # a tile past the cap sends the next batch down the plan path, with the same verdicts
    np.testing.assert_array_equal(probe(fresh, m), want)
    assert paths(fresh) == ((1, 1) if total > TILE_CAP else (2, 0))


def test_hot_batch_takes_the_plan_path_for_64_batches(fresh, oracle_mod):
    w = window(5)
    hot = placed_batch(w, one_tile_total(w, 5000), seed=5000)   # rounds 1024 x 4 + 904; G = 2
    cool = placed_batch(w, round_robin(2000, 5), seed=2000)
    tm = ingest(fresh, w)
    want_hot, want_cool = reference(w, oracle_mod, hot, tm), reference(w, oracle_mod, cool, tm)
    for want in (want_hot, want_cool):
        assert 0 < int(want.sum()) < len(want)
    np.testing.assert_array_equal(probe(fresh, cool), want_cool)
    assert paths(fresh) == (1, 0)
    # the first concentrated batch runs its rounds inside the tile's block ...
    np.testing.assert_array_equal(probe(fresh, hot), want_hot)
    assert paths(fresh) == (2, 0)
    # ... the same batch again takes the plan and its overflow blocks (and reports itself hot)
    np.testing.assert_array_equal(probe(fresh, hot), want_hot)
    assert paths(fresh) == (2, 1)
    # the 64 batches after the last hot one stay there, the next one is back
    u = upload(cool)
    out = outputs(cool)
    torch.cuda.synchronize()
    for k in range(HOT_BATCHES):
        launch(fresh, cool, u, out)
        torch.cuda.synchronize()
        assert paths(fresh) == (2, 2 + k)
    np.testing.assert_array_equal(result(cool, *out), want_cool)
    np.testing.assert_array_equal(probe(fresh, cool), want_cool)
    assert paths(fresh) == (3, 1 + HOT_BATCHES)


# ---- verdict plumbing ------------------------------------------------------------
KINDS = ("locate", "lock", "join", "quiet", "quiet-lock")


def plumbing_batch(w, n_txn, every, seed, conflicts=True):
    """Read set t with t % every == 0 is of kind KINDS[(t // every) % 5]; the
    others have no range and no lock (their verdict bytes must come back 0).
      locate      tile a exactly and the first three rows of tile a + 1, whose
                  newest commit is the snapshot and older than tile a's: the
                  locate's whole-tile check of tile a finds the conflict, the
                  join record in tile a + 1 finds none
      lock        a table lock, snapshot before every commit
      join        a narrow range whose snapshot is the LSN before its newest row
      quiet       a narrow range, snapshot after every commit
      quiet-lock  a table lock, snapshot after every commit
    conflicts=False: every snapshot after every commit."""
    rng = np.random.default_rng(seed)
    t = np.arange(0, n_txn, every)
    kind = (t // every) % 5
    before = np.uint64(NEVER if not conflicts else LSN0 - 1)
    lo, hi, snap, txn = [], [], [], []
    sel = t[kind == 0]
    tmax = np.array([w.lsn[x * TILE:(x + 1) * TILE].max() for x in range(w.ntiles - 1)])
    head = np.array([w.lsn[x * TILE:x * TILE + 3].max() for x in range(1, w.ntiles)])
    cand = np.flatnonzero(tmax > head)
    assert len(cand)
    a = cand[rng.integers(0, len(cand), len(sel))]
    lo.append(w.keys[a * TILE]), hi.append(w.keys[(a + 1) * TILE + 2] + 1)
    snap.append(head[a] if conflicts else np.full(len(sel), np.uint64(NEVER))), txn.append(sel)
    for kd in (2, 3):
        sel = t[kind == kd]
        l, h, s = narrow_ranges(w, rng.integers(0, w.ntiles, len(sel)), seed + kd,
                                "all" if kd == 2 and conflicts else "none", empties=False)
        lo.append(l), hi.append(h), snap.append(s), txn.append(sel)
    lock_txn = np.concatenate([t[kind == 1], t[kind == 4]])
    lock_snap = np.concatenate([np.full(int((kind == 1).sum()), before),
                                np.full(int((kind == 4).sum()), np.uint64(NEVER))])
    cat = np.concatenate
    return kind, batch(cat(lo), cat(hi), cat(snap), cat(txn), n_txn, lock_snap, lock_txn)


@pytest.mark.parametrize("bitmap", [True, False], ids=["bitmap", "bytes"])
def test_verdict_plumbing(fresh, oracle_mod, bitmap):
    """5 tiles: the join's grid is 8 blocks of 512 threads, one stride of its
    flag move 4096 read sets; 24613 read sets = the hoisted stride, a full
    group of four and a partial one."""
    w = window(5)
    tm = ingest(fresh, w)
    assert len(tm) == 1 and LSN0 <= int(tm[0]) < NEVER
    # one read set: a conflict found only by the join, and none
    for conflicts in (True, False):
        l, h, s = narrow_ranges(w, [3], seed=9, conflicts="all" if conflicts else "none", empties=False)
        m = batch(l, h, s, [0], 1)
        want = reference(w, oracle_mod, m, tm)
        assert bool(want[0]) == conflicts
        np.testing.assert_array_equal(probe(fresh, m, bitmap), want)
    done = 2
    for n_txn, every in ((63, 1), (64, 1), (65, 1), (24613, 8)):
        kind, m = plumbing_batch(w, n_txn, every, seed=n_txn)
        want = reference(w, oracle_mod, m, tm)
        assert 0 < int(want.sum()) < n_txn
        # every kind does what its name says
        by_kind = [want[::every][kind == k] for k in range(5)]
        assert all(by_kind[k].all() for k in (0, 1, 2)) and not any(by_kind[k].any() for k in (3, 4))
        np.testing.assert_array_equal(probe(fresh, m, bitmap), want)
        # the same context again, nothing conflicts: a flag left set would show
        _, quiet = plumbing_batch(w, n_txn, every, seed=n_txn, conflicts=False)
        assert not reference(w, oracle_mod, quiet, tm).any()
        assert not probe(fresh, quiet, bitmap).any()
        done += 2
    assert paths(fresh) == (done, 0)


@pytest.mark.parametrize("nstreams", [2, 3])
def test_streams_interleaved(fresh, oracle_mod, nstreams):
    dev = torch.device("cuda", 0)
    w = window(33)
    tm = ingest(fresh, w)
    ms = [placed_batch(w, round_robin(8 * CHUNK - 5 - 1000 * k, 33), seed=70 + k) for k in range(2)]
    want = [reference(w, oracle_mod, m, tm) for m in ms]
    for x in want:
        assert 0 < int(x.sum()) < len(x)
    ups = [upload(m) for m in ms]
    streams = [torch.cuda.Stream(device=dev) for _ in range(nstreams)]
    order = [(k % nstreams, (k // nstreams + k) % 2) for k in range(4 * nstreams)]
    outs = [(bi, outputs(ms[bi])) for _, bi in order]  # one pair per launch: nothing but the lanes is shared
    torch.cuda.synchronize()
    try:
        for (si, bi), (_, out) in zip(order, outs):
            fresh.set_stream(streams[si].cuda_stream)
            launch(fresh, ms[bi], ups[bi], out)
        torch.cuda.synchronize()
    finally:
        fresh.set_stream(0)
    for bi, (verdict, bits) in outs:
        np.testing.assert_array_equal(result(ms[bi], verdict, bits), want[bi])
    assert paths(fresh) == (4 * nstreams, 0)
