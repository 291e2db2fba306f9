"""A plain numpy model of the rows appended after a window build, and the
generators of the placed appended-row tests (tests/test_appended_model.py on
the CPU, tests/test_gpu_appended_placed.py on the GPU).

The library keeps appended rows (gid, words[W], lsn) apart from the main
window: a run sorted by (gid, words) with stable ties (k_delta_merge,
comdb2_amd/csrc/hsc_delta.hip: equal keys keep the older rows first) with
64-row LSN maxima, and a short pending tail in append order.  A range probe
(g, lo, hi, snap) conflicts when any row of the main window or of the
appended rows has gid == g, lo <= words <= hi and lsn > snap; a read set's
verdict is the OR over its ranges and table locks.

The model holds both sets of rows and answers, per range: pa / pb (the rows of
the sorted run below lo / not above hi), the LSN maximum over the union of
rows, and the verdicts of a marshalled batch (Validator.marshal layout).

The generators place their probes.  Append number j carries the commit LSN
END + j (hsc_window_append wants non-decreasing commit LSNs), every main-window
LSN is below END, and no snapshot is below END - 1: a verdict is the appended
rows' alone.  Keys are given to the append order by a fixed scramble, or by
ranks the generator chooses, so every row range of the sorted run has one
known newest row; a probe's snapshot is that row's LSN (no conflict) or the
LSN before it (a conflict).
"""

import numpy as np

KEY0, KEY_STEP = 1000, 7        # main window: distinct int64 keys KEY0 + KEY_STEP i
APP0, APP_STEP = KEY0 - 20, 3   # appended int64 keys: between the main keys and onto some
LSN0 = (5 << 32) + 4096         # oldest main-window commit
LSN_MOD = 1 << 20
END = LSN0 + LSN_MOD            # append j commits at END + j
BLOCK = 64                      # rows per LSN maximum of a run
INT64_KLEN = 9                  # bytes of an encoded int64 key (two words)


# ---- keys -------------------------------------------------------------------
def int64_words(vals):
    """int64 key values -> uint64[2][n]: the big-endian words of their 9-byte
    keys (a 0x08 header, the value with its sign bit flipped), zero padded."""
    v = np.asarray(vals, np.int64).view(np.uint64) ^ np.uint64(1 << 63)
    w0 = (np.uint64(0x08) << np.uint64(56)) | (v >> np.uint64(8))
    w1 = (v & np.uint64(0xFF)) << np.uint64(56)
    return np.stack([w0, w1])


def words_bytes(words, klen):
    """uint64[W][n] key words -> uint8[n][klen] key bytes."""
    words = np.asarray(words, np.uint64)
    W, n = words.shape
    b = np.ascontiguousarray(words.T).astype(">u8").view(np.uint8).reshape(n, 8 * W)
    assert not b[:, klen:].any(), "key words set past the key length"
    return np.ascontiguousarray(b[:, :klen])


def row_keys(gid, words):
    """Composite keys (gid, words[W][n]) as fixed-width byte strings: they
    sort, search and compare as the composites do."""
    words = np.asarray(words, np.uint64)
    W, n = words.shape
    b = np.empty((n, 4 + 8 * W), np.uint8)
    b[:, :4] = np.asarray(gid, np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)
    b[:, 4:] = np.ascontiguousarray(words.T).astype(">u8").view(np.uint8).reshape(n, 8 * W)
    return b.view(f"S{4 + 8 * W}").reshape(n)


def scramble(n):
    """A fixed permutation of 0 .. n-1 (the append rank of sorted row i)."""
    i = np.arange(n, dtype=np.uint64)
    h = (i * np.uint64(2654435761) + (i >> np.uint64(12)) * np.uint64(40503)) % np.uint64(1 << 32)
    rank = np.empty(n, np.int64)
    rank[np.argsort(h, kind="stable")] = np.arange(n)
    return rank


class Rows:
    """Rows (gid u32[n], words u64[W][n], lsn u64[n])."""

    def __init__(self, gid, words, lsn):
        self.gid = np.ascontiguousarray(gid, np.uint32)
        self.words = np.ascontiguousarray(words, np.uint64)
        self.lsn = np.ascontiguousarray(lsn, np.uint64)
        assert self.words.ndim == 2 and self.words.shape[1] == len(self.gid) == len(self.lsn)

    def __len__(self):
        return len(self.lsn)

    @staticmethod
    def empty(W):
        return Rows(np.zeros(0, np.uint32), np.zeros((W, 0), np.uint64), np.zeros(0, np.uint64))

    def take(self, idx):
        return Rows(self.gid[idx], self.words[:, idx], self.lsn[idx])

    def cat(self, other):
        return Rows(np.concatenate([self.gid, other.gid]), np.concatenate([self.words, other.words], axis=1),
                    np.concatenate([self.lsn, other.lsn]))

    def sorted(self):
        """Key order, stable: equal keys keep their order (older first)."""
        return self.take(np.argsort(row_keys(self.gid, self.words), kind="stable"))


class Model:
    """The main-window rows and the appended rows (in append order)."""

    def __init__(self, W, main=None):
        self.W = W
        self.main = main if main is not None else Rows.empty(W)
        assert self.main.words.shape[0] == W
        self.app = Rows.empty(W)
        self._union = None

    def append(self, rows):
        assert rows.words.shape[0] == self.W
        seq = np.concatenate([self.app.lsn[-1:], rows.lsn])
        assert (seq[1:] >= seq[:-1]).all(), "commit LSNs must not decrease"
        self.app = self.app.cat(rows)
        self._union = None

    def run(self, count=None, first=0):
        """The sorted run of appended rows [first, first + count) (all by default)."""
        count = len(self.app) - first if count is None else count
        return self.app.take(np.arange(first, first + count)).sorted()

    def union(self):
        if self._union is None:
            u = self.main.cat(self.app).sorted()
            self._union = (u, row_keys(u.gid, u.words))
        return self._union

    @staticmethod
    def positions(rows, gid, lo, hi):
        """(pa, pb) per range over sorted `rows`: rows below (gid, lo) and rows
        not above (gid, hi); the range's rows are [pa, pb)."""
        k = row_keys(rows.gid, rows.words)
        return (np.searchsorted(k, row_keys(gid, lo), "left").astype(np.int64),
                np.searchsorted(k, row_keys(gid, hi), "right").astype(np.int64))

    @staticmethod
    def _max_of(lsn, pa, pb):
        out = np.zeros(len(pa), np.uint64)
        ok = pb > pa
        if ok.any():
            pad = np.concatenate([lsn, np.zeros(1, np.uint64)])
            idx = np.stack([pa[ok], pb[ok]], axis=1).reshape(-1)
            out[ok] = np.maximum.reduceat(pad, idx)[::2]
        return out

    def range_max(self, gid, lo, hi, rows=None):
        """Newest LSN per range over the union of rows (or `rows`, sorted); 0: no row."""
        if rows is None:
            rows, k = self.union()
        else:
            k = row_keys(rows.gid, rows.words)
        pa = np.searchsorted(k, row_keys(gid, lo), "left")
        pb = np.searchsorted(k, row_keys(gid, hi), "right")
        return self._max_of(rows.lsn, pa, pb)

    def table_max(self, group_table, ntables):
        """Newest LSN per table over the union (group_table[g] = table of group g)."""
        u, _ = self.union()
        out = np.zeros(ntables, np.uint64)
        np.maximum.at(out, np.asarray(group_table)[u.gid], u.lsn)
        return out

    def verdicts(self, m, table_max=None, rows=None):
        """bool[n_txn] of a marshalled batch: per read set the OR of its ranges
        (a row of the union, or of `rows`, newer than the snapshot), its table
        locks (the table's newest LSN newer than the lock's snapshot) and its
        host-forced verdict."""
        out = np.zeros(m["n_txn"], bool)
        out[:len(m["forced"])] = np.asarray(m["forced"]) != 0
        if m["n"]:
            hit = self.range_max(m["gid"], m["lo"], m["hi"], rows) > np.asarray(m["snap"], np.uint64)
            np.logical_or.at(out, np.asarray(m["txn"], np.int64), hit)
        if m["n_lock"]:
            hit = np.asarray(table_max, np.uint64)[m["lock_table"]] > np.asarray(m["lock_snap"], np.uint64)
            np.logical_or.at(out, np.asarray(m["lock_txn"], np.int64), hit)
        return out

    def verdicts_brute(self, m, table_max=None):
        """The same by the definition, row by row (small batches)."""
        out = np.zeros(m["n_txn"], bool)
        out[:len(m["forced"])] = np.asarray(m["forced"]) != 0
        rows = self.main.cat(self.app)
        keys = [tuple(int(x) for x in rows.words[:, r]) for r in range(len(rows))]
        for q in range(m["n"]):
            lo = tuple(int(x) for x in m["lo"][:, q])
            hi = tuple(int(x) for x in m["hi"][:, q])
            g, s = int(m["gid"][q]), int(m["snap"][q])
            if any(int(rows.gid[r]) == g and lo <= keys[r] <= hi and int(rows.lsn[r]) > s
                   for r in range(len(rows))):
                out[m["txn"][q]] = True
        for q in range(m["n_lock"]):
            if int(table_max[m["lock_table"][q]]) > int(m["lock_snap"][q]):
                out[m["lock_txn"][q]] = True
        return out


# ---- probe columns -----------------------------------------------------------
def batch(W, gid, lo, hi, snap, lock_table=(), lock_snap=()):
    """Probe columns in the marshalled layout: read set t is range t, the read
    sets after the ranges one table lock each."""
    n, nl = len(snap), len(lock_snap)
    return dict(words=W, n=n, n_lock=nl, n_txn=n + nl,
                lo=np.ascontiguousarray(lo, np.uint64).reshape(W, n),
                hi=np.ascontiguousarray(hi, np.uint64).reshape(W, n),
                gid=np.ascontiguousarray(gid, np.uint32), snap=np.ascontiguousarray(snap, np.uint64),
                txn=np.arange(n, dtype=np.uint32),
                lock_table=np.ascontiguousarray(lock_table, np.uint32),
                lock_snap=np.ascontiguousarray(lock_snap, np.uint64),
                lock_txn=np.arange(n, n + nl, dtype=np.uint32), forced=np.zeros(n + nl, np.uint8))


def cat_batches(ms):
    """Several range-only batches of one width as one."""
    W = ms[0]["words"]
    assert all(m["n_lock"] == 0 and m["words"] == W for m in ms)
    cat = np.concatenate
    return batch(W, cat([m["gid"] for m in ms]), cat([m["lo"] for m in ms], axis=1),
                 cat([m["hi"] for m in ms], axis=1), cat([m["snap"] for m in ms]))


def slice_batch(m, a, b):
    """Ranges (= read sets) [a, b) of a range-only batch."""
    assert m["n_lock"] == 0
    return batch(m["words"], m["gid"][a:b], m["lo"][:, a:b], m["hi"][:, a:b], m["snap"][a:b])


# ---- the main window ---------------------------------------------------------
def main_keys(n):
    return KEY0 + KEY_STEP * np.arange(n, dtype=np.int64)


def main_lsn(n):
    """A fixed scramble of the row index below END: old and new rows everywhere."""
    i = np.arange(n, dtype=np.uint64)
    return np.uint64(LSN0) + (i * np.uint64(2654435761) + (i >> np.uint64(12)) * np.uint64(40503)) % np.uint64(LSN_MOD)


def main_window(n, gid=0):
    """n rows of distinct int64 keys with stride KEY_STEP in group `gid`."""
    return Rows(np.full(n, gid, np.uint32), int64_words(main_keys(n)), main_lsn(n))


def app_keys(n):
    return APP0 + APP_STEP * np.arange(n, dtype=np.int64)


def ranked_appends(gid, words, rank, first=0):
    """Rows given in any order with distinct append ranks -> Rows in append
    order, row of rank r committing at END + first + r."""
    order = np.argsort(rank, kind="stable")
    assert (np.sort(rank) == np.arange(len(rank))).all()
    lsn = np.uint64(END + first) + np.arange(len(rank), dtype=np.uint64)
    return Rows(np.asarray(gid, np.uint32)[order], np.asarray(words, np.uint64)[:, order], lsn)


# ---- (a) search positions ------------------------------------------------------
class SearchCase:
    """A run of n int64 keys APP0 + APP_STEP i in group 0 over a main window of
    `nmain` rows; sorted row i has the append rank scramble(n)[i]."""

    def __init__(self, n, nmain=4096 + 777):
        self.n, self.W = n, 2
        self.main = main_window(nmain)
        self.keys = app_keys(n)
        self.rank = scramble(n)
        self.lsn = np.uint64(END) + self.rank.astype(np.uint64)  # of sorted row i
        self.appends = ranked_appends(np.zeros(n, np.uint32), int64_words(self.keys), self.rank)

    def model(self):
        m = Model(2, self.main)
        m.append(self.appends)
        return m

    def probes(self, rows):
        """Per row i of `rows`: [K_i, K_i] at the row's LSN (no conflict) and the
        LSN before (a conflict), and the empty range [K_i + 1, K_i + 2] at the
        oldest snapshot in use (END - 1: any appended row leaking in conflicts)."""
        rows = np.asarray(rows, np.int64)
        k = self.keys[rows]
        lo = np.concatenate([k, k, k + 1])
        hi = np.concatenate([k, k, k + 2])
        snap = np.concatenate([self.lsn[rows], self.lsn[rows] - np.uint64(1),
                               np.full(len(rows), END - 1, np.uint64)])
        # interleave: consecutive read sets are one row's three probes
        order = np.arange(3 * len(rows)).reshape(3, len(rows)).T.reshape(-1)
        return batch(2, np.zeros(len(lo), np.uint32), int64_words(lo[order]), int64_words(hi[order]), snap[order])

    def boundary_rows(self, extra=2048):
        """Rows within 2 of a multiple of 16 (256 and 4096 among them), the
        last rows, and `extra` others."""
        i = np.arange(self.n)
        near = (i % 16 <= 2) | (i % 16 >= 14) | (i >= self.n - 3)
        rest = np.flatnonzero(~near)
        step = max(1, len(rest) // extra)
        near[rest[::step][:extra]] = True
        return np.flatnonzero(near)


SEARCH_SIZES = (1, 2, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097)


# ---- (b) head / whole blocks / tail ----------------------------------------------
OFFSETS = (0, 1, 63)        # pa % 64 and pb % 64
WHOLE = (0, 1, 2, 5)        # whole 64-row blocks between head and tail
NEWEST = ("first", "last", "last-head", "block-first", "block-last", "first-tail")


def _newest_row(where, pa, hend, bend, pb):
    """The row of [pa, pb) (head [pa, hend), blocks [hend, bend), tail [bend,
    pb)) named by `where`, or None where the range has no such part."""
    if where == "first":
        return pa
    if where == "last":
        return pb - 1
    if where == "last-head":
        return hend - 1 if hend > pa else None
    if where == "block-first":
        return hend if bend > hend else None
    if where == "block-last":
        return bend - 1 if bend > hend else None
    return bend if pb > bend else None  # first-tail


class BlockCase:
    """One run holding a region per (pa % 64, pb % 64, whole blocks, newest
    row): rows [pa, pb) of the sorted run with the range's newest row where the
    class says, and the rows pa - 1 and pb newer than every snapshot used.

    Append ranks: ordinary rows first (scrambled), then the ranges' newest rows,
    then the guard rows pa - 1 and pb.  `limit` keeps the regions that end
    within the first `limit` rows (a run cut short has its own newest rows)."""

    def __init__(self, nmain=4096 + 777, limit=None, only_whole=None, first_row=0):
        regs, at = [], BLOCK * ((first_row + BLOCK - 1) // BLOCK)
        for B in (WHOLE if only_whole is None else only_whole):
            for a in OFFSETS:
                for b in OFFSETS:
                    for where in NEWEST:
                        pa = at + BLOCK + a
                        hend = (pa + BLOCK - 1) // BLOCK * BLOCK
                        bend = hend + BLOCK * B
                        pb = bend + b
                        if pb <= pa:
                            continue
                        r = _newest_row(where, pa, hend, bend, pb)
                        if r is None:
                            continue
                        if limit is not None and pb + 1 > limit:
                            continue
                        regs.append((a, b, B, where, pa, pb, r))
                        at = (pb + 1 + BLOCK - 1) // BLOCK * BLOCK
        self.regions = regs
        self.n = n = (at + BLOCK) if limit is None else limit
        self.W = 2
        self.main = main_window(nmain)
        self.keys = app_keys(n)
        cls = np.zeros(n, np.int64)
        for *_, pa, pb, r in regs:
            cls[r] = 1
        for *_, pa, pb, r in regs:
            cls[pa - 1] = 2
            cls[pb] = 2
        self.rank = np.empty(n, np.int64)
        self.rank[np.lexsort((scramble(n), cls))] = np.arange(n)
        self.lsn = np.uint64(END) + self.rank.astype(np.uint64)
        self.appends = ranked_appends(np.zeros(n, np.uint32), int64_words(self.keys), self.rank)
        self.guard_min = int(self.lsn[cls == 2].min()) if (cls == 2).any() else None

    def model(self):
        m = Model(2, self.main)
        m.append(self.appends)
        return m

    def probes(self):
        """Per region two read sets: [K_pa - 1, K_{pb-1} + 1] (between keys: no
        further row) at the newest row's LSN and at the LSN before it."""
        pa = np.array([r[4] for r in self.regions])
        pb = np.array([r[5] for r in self.regions])
        nw = np.array([r[6] for r in self.regions])
        lo = np.repeat(self.keys[pa] - 1, 2)
        hi = np.repeat(self.keys[pb - 1] + 1, 2)
        snap = np.repeat(self.lsn[nw], 2)
        snap[1::2] -= np.uint64(1)
        return batch(2, np.zeros(len(lo), np.uint32), int64_words(lo), int64_words(hi), snap)


def whole_blocks(pa, pb):
    hend = np.minimum(pb, (pa + BLOCK - 1) // BLOCK * BLOCK)
    bend = pb // BLOCK * BLOCK
    return np.maximum(bend - hend, 0) // BLOCK


# ---- (c) groups and key words -------------------------------------------------------
WIDTHS = (1, 2, 4, 5, 9)
VARY = ("first-word", "last-word", "last-bytes")


def key_len(W, vary):
    """Key bytes of the case's groups: whole words, or ("last-bytes") three
    bytes short of them -- the last word ends in zero padding."""
    return 8 * W - 3 if vary == "last-bytes" else 8 * W


def vary_words(W, vary, vals):
    """uint64[W][n]: every key the same fixed bytes but for `vals` (< 2^24),
    held by the first word, by the last word, or by the last three key bytes
    before the padding."""
    vals = np.asarray(vals, np.uint64)
    assert int(vals.max(initial=0)) < 1 << 24
    w = np.empty((W, len(vals)), np.uint64)
    for j in range(W):
        w[j] = np.uint64(0x4142434445464700 + 0x0101010101010100 * j)
    if vary == "first-word":
        w[0] = np.uint64(0x4142434400000000) | vals
    elif vary == "last-word":
        w[W - 1] = np.uint64(0x5152535400000000) | vals
    else:  # bytes klen-3 .. klen-1 = bytes 2..4 of the last word; 5..7 are padding
        w[W - 1] = np.uint64(0x6162000000000000) | (vals << np.uint64(24))
    return w


class GroupCase:
    """Three groups 0, 1, 2 hold the same key words (values 20 + 3 i) with
    different LSNs, in a run over a main window of keys 7 i in every group.
    Probes ask group 1 only."""

    def __init__(self, W, vary, n=300, nmain=500):
        self.W, self.vary, self.n = W, vary, n
        self.klen = key_len(W, vary)
        mv = KEY_STEP * np.arange(nmain)
        self.main = Rows(np.repeat(np.arange(3, dtype=np.uint32), nmain),
                         np.tile(vary_words(W, vary, mv), 3), main_lsn(3 * nmain))
        self.vals = 20 + APP_STEP * np.arange(n)
        gid = np.repeat(np.arange(3, dtype=np.uint32), n)
        words = np.tile(vary_words(W, vary, self.vals), 3)
        self.rank = scramble(3 * n)
        self.lsn = (np.uint64(END) + self.rank.astype(np.uint64)).reshape(3, n)  # [group][row]
        self.appends = ranked_appends(gid, words, self.rank)

    def model(self):
        m = Model(self.W, self.main)
        m.append(self.appends)
        return m

    def probes(self):
        """Group 1: every row alone at its LSN and the LSN before, and ranges of
        1 .. 40 rows -- every seventh of 130 .. 250 rows, over whole 64-row
        blocks of the run -- at their newest LSN and the LSN before."""
        n = self.n
        i = np.arange(n)
        a = (i * 7) % (n - 41)
        b = a + 1 + i % 40
        long = i % 7 == 3
        a[long] = (i[long] * 11) % (n - 251)
        b[long] = a[long] + 130 + i[long] % 121
        l1 = self.lsn[1]
        rmax = np.array([l1[x:y].max() for x, y in zip(a, b)], np.uint64)
        lo = np.concatenate([self.vals[i], self.vals[i], self.vals[a], self.vals[a]])
        hi = np.concatenate([self.vals[i], self.vals[i], self.vals[b - 1], self.vals[b - 1]])
        snap = np.concatenate([l1, l1 - np.uint64(1), rmax, rmax - np.uint64(1)])
        return batch(self.W, np.ones(len(lo), np.uint32), vary_words(self.W, self.vary, lo),
                     vary_words(self.W, self.vary, hi), snap)


# ---- (d) the pending tail ---------------------------------------------------------
PENDING_SIZES = (1, 2, 255, 256)


class PendingCase(SearchCase):
    """n rows appended a few at a time, staying in the pending tail: probes of
    every row as SearchCase.probes, ranges whose bound is a pending key on
    either side, and table locks at the newest pending LSN and the one before."""

    def pieces(self):
        """Append sizes: 1, 2, 3, ... rows per append."""
        out, k = [], 0
        while sum(out) < self.n:
            k += 1
            out.append(min(k, self.n - sum(out)))
        return out

    def bound_probes(self):
        """Per row i: [K_i - 2, K_i] and [K_i, K_i + 2] hold row i alone (a
        bound equal to the key), [K_i - 2, K_i - 1] and [K_i + 1, K_i + 2] no row."""
        k = self.keys
        n = self.n
        lo = np.concatenate([k - 2, k - 2, k, k, k - 2, k + 1])
        hi = np.concatenate([k, k, k + 2, k + 2, k - 1, k + 2])
        one = np.uint64(1)
        snap = np.concatenate([self.lsn, self.lsn - one, self.lsn, self.lsn - one,
                               np.full(2 * n, END - 1, np.uint64)])
        return batch(2, np.zeros(len(lo), np.uint32), int64_words(lo), int64_words(hi), snap)

    def lock_probes(self, table=0):
        top = END + self.n - 1
        return batch(2, np.zeros(0, np.uint32), np.zeros((2, 0), np.uint64), np.zeros((2, 0), np.uint64),
                     np.zeros(0, np.uint64), [table, table], [top, top - 1])


# ---- block-boundary ranges of any run -------------------------------------------------
def boundary_probes(run, W, bases=8):
    """Ranges of the sorted run `run` (one group) around its 64-row blocks: rows
    [pa, pb) with pa % 64 and pb % 64 in OFFSETS over 0, 1, 2 and 5 whole
    blocks, from up to `bases` block starts spread over the run, the bounds
    equal to the end rows' keys.  Equal keys next to an end widen the range, so
    the snapshots come from the rows the bounds really hold: the newest LSN
    among them and the LSN before it.  -> (batch, pa, pb)."""
    n = len(run)
    nblk = n // BLOCK + 1
    picks = sorted({int(x) for x in np.linspace(0, max(nblk - 1, 0), bases)})
    pa_l, pb_l = [], []
    for s in picks:
        for B in WHOLE:
            for a in OFFSETS:
                for b in OFFSETS:
                    pa = BLOCK * s + a
                    pb = (pa + BLOCK - 1) // BLOCK * BLOCK + BLOCK * B + b
                    if pa < pb <= n:
                        pa_l.append(pa), pb_l.append(pb)
    if n and not pa_l:
        pa_l, pb_l = [0], [n]
    pa, pb = np.array(pa_l, np.int64), np.array(pb_l, np.int64)
    gid = np.repeat(run.gid[pa], 2)
    lo, hi = np.repeat(run.words[:, pa], 2, axis=1), np.repeat(run.words[:, pb - 1], 2, axis=1)
    ra, rb = Model.positions(run, gid, lo, hi)
    snap = Model._max_of(run.lsn, ra, rb)
    snap[1::2] -= np.uint64(1)
    return batch(W, gid, lo, hi, snap), ra, rb


# ---- (e) merge variants, (g) folds: a stream of appends with repeated keys --------------
# run sizes before an append 0, 63, 64, 65 and 256; appends of 1, 255, 256, 257 and 3000 rows
MERGE_STEPS = (63, 1, 1, 191, 255, 256, 257, 3000)
FOLD_STEPS = (250,) * 9         # folds at 600 rows: after the 3rd, 6th and 9th append


class StreamCase:
    """Appends of the given sizes in group 0: append j writes the int64 key
    APP0 + APP_STEP ((j * 7919) % M), M = 85 % of the rows, so about one key in
    seven comes again later (its newer version follows the older one in the
    run) and every seventh of them is a main-window key too."""

    def __init__(self, steps, nmain=4096 + 777, first=0):
        self.steps, self.W = tuple(steps), 2
        self.main = main_window(nmain)
        n = sum(steps)
        j = np.arange(n, dtype=np.int64)
        self.keys = APP0 + APP_STEP * ((j * 7919) % max(1, n * 85 // 100))  # in append order
        self.rows = Rows(np.zeros(n, np.uint32), int64_words(self.keys),
                         np.uint64(END + first) + j.astype(np.uint64))

    def pieces(self):
        at = 0
        for k in self.steps:
            yield self.rows.take(np.arange(at, at + k))
            at += k


# ---- (f) the device probe with a run: main window, run, both, neither ------------------
KINDS = ("main", "run", "both", "neither", "none", "lock")
DEVICE_TXNS = (1, 63, 64, 65, 4097)


class DeviceCase:
    """A main window and a run of distinct keys (some of them main-window keys
    too; sorted run row i has the append rank scramble(n)[i]).  Read set t is of
    kind KINDS[(t + 1) % 6]:
      main     one main-window key the run does not hold, at the LSN before the
               row's (older than END: the only case whose snapshots are)
      run      one run key the main window does not hold, at the LSN before the row's
      both     one key of both, at the LSN before the older (main-window) row's
      neither  one run key at its run row's LSN
      none     no range and no lock
      lock     the table, at its newest LSN (no conflict) or the one before"""

    def __init__(self, main, run_gid, run_words):
        self.main = main.sorted()
        self.W = main.words.shape[0]
        self.n = n = len(run_gid)
        self.run = Rows(run_gid, run_words, np.uint64(END) + scramble(n).astype(np.uint64))
        rk, mk = row_keys(self.run.gid, self.run.words), row_keys(self.main.gid, self.main.words)
        assert (rk[1:] > rk[:-1]).all() and (mk[1:] > mk[:-1]).all()
        self.appends = ranked_appends(run_gid, run_words, scramble(n))
        on_main = np.isin(rk, mk)
        self.pools = {"main": np.flatnonzero(~np.isin(mk, rk)), "run": np.flatnonzero(~on_main),
                      "both": np.flatnonzero(on_main), "neither": np.arange(n)}
        self.main_of = np.searchsorted(mk, rk)  # (of the rows in "both")
        assert all(len(p) for p in self.pools.values())

    def model(self):
        m = Model(self.W, self.main)
        m.append(self.appends)
        return m

    def batch(self, T, seed=0):
        t = np.arange(T)
        kind = (t + 1) % 6
        gid, words, snap, txn = [], [], [], []
        one = np.uint64(1)
        for k, name in enumerate(KINDS[:4]):
            sel = t[kind == k]
            pool = self.pools[name]
            r = pool[(sel * 7919 + seed) % len(pool)]
            src = self.main if name == "main" else self.run
            gid.append(src.gid[r]), words.append(src.words[:, r]), txn.append(sel)
            snap.append({"main": lambda: self.main.lsn[r] - one, "run": lambda: self.run.lsn[r] - one,
                         "both": lambda: self.main.lsn[self.main_of[r]] - one,
                         "neither": lambda: self.run.lsn[r]}[name]())
        cat = np.concatenate
        w = cat(words, axis=1)
        lt = t[kind == 5]
        top = END + self.n - 1
        m = batch(self.W, cat(gid), w, w, cat(snap), np.zeros(len(lt), np.uint32), top - (lt // 6) % 2)
        m["txn"], m["lock_txn"] = cat(txn).astype(np.uint32), lt.astype(np.uint32)
        m["n_txn"], m["forced"] = T, np.zeros(T, np.uint8)
        return m, kind


def int64_device_case(nmain=2 * 4096 + 777, n=1500):
    """Three narrow tiles of int64 keys and a run over the first tile's keys."""
    return DeviceCase(main_window(nmain), np.zeros(n, np.uint32), int64_words(app_keys(n)))


def compact_device_case(nmain=6000, n=1500):
    """23-byte keys of few varying bits per byte (0x00, 0x08, 0x61, 0x62 in 22
    places: 110 varying bits, past the narrow codes, within three words of
    compact codes), a third of the run's keys main-window keys too."""
    rng = np.random.default_rng(23)
    kb = np.zeros((nmain + n, 24), np.uint8)
    kb[:, 0] = 8
    kb[:, 1:23] = rng.choice(np.array([0x00, 0x08, 0x61, 0x62], np.uint8), (nmain + n, 22))
    words = np.ascontiguousarray(kb.view(">u8").astype(np.uint64).T)
    keys = row_keys(np.zeros(nmain + n, np.uint32), words)
    assert len(np.unique(keys)) == nmain + n
    mw = words[:, :nmain]
    rw = np.concatenate([words[:, nmain + n // 3:], mw[:, ::nmain // (n // 3)][:, :n // 3]], axis=1)
    rw = rw[:, np.argsort(row_keys(np.zeros(n, np.uint32), rw))]
    return DeviceCase(Rows(np.zeros(nmain, np.uint32), mw, main_lsn(nmain)), np.zeros(n, np.uint32), rw)
