"""An integer model of the compact-code probes, and the generator of the placed
compact-bound tests (tests/test_compact_placed_model.py on the CPU,
tests/test_gpu_compact_placed.py on the GPU).

A wide window that is not narrow is probed through compact codes: every
(table, index, key length) group keeps only the key bits that vary inside it,
and a probe bound is mapped onto those codes by the rules at the top of
comdb2_amd/csrc/hsc_compact.hip -- in bound_codes / bound_map
(hsc_compact_dev.h, keys of at most 8 words), in code_of (longer keys, and the
window rows), through the point index (k_ph_insert / ph_find / ph_key), and in
cnarrow_bound (hsc_narrow.hip) when the varying bits total <= 62.

Keys are Python integers of 64 W bits (word 0 the most significant).  A group
is built from a pattern C and a varying mask M: its rows are C, C | M, rows
with a single varying bit, the anchors of the carry / borrow bounds and seeded
random subsets of M, so the device derives exactly M.  LSNs are distinct and
scrambled against key order.

The model (Model.verdicts) is the definition and nothing else: read set t
conflicts iff some row of its group has lo <= row <= hi as integers and
lsn > snap.

Bounds are placed by branch of the mapping rule: each bound X carries the tag
of the branch it is meant to hit (TAGS), classify() computes the tags a bound
really has from (X, C, M).  Every bound is used as lo and as hi: with its
neighbouring rows pred < X < succ it gives the ranges [X, succ] and [pred, X]
at the far row's LSN (no conflict, unless the model finds another row) and at
the LSN before (a conflict), the empty ranges [X, pred] and [succ, X], the
point [X, X], and [X, max] and [0, X] at a snapshot before every row.  A batch
holds one range per read set, so nothing is OR-ed away, and comes in three
orders (ORDERS).
"""

import bisect
import functools

import numpy as np

import appended_model as A

M64 = (1 << 64) - 1
LSN0 = A.LSN0 + 16              # oldest commit of every window here
BEFORE = A.LSN0 - 1             # a snapshot before every row
ORDERS = ("points-first", "alternating", "shuffle")

POS = ("np0", "between", "k0", "bit63", "bit0", "zero-mask-word", "last-word")
PRE = ("zeros", "ones", "generic", "carry", "borrow")
TAGS = (("exact-present", "exact-absent", "zero", "max") +
        tuple(f"pos:{p}/x{x}" for p in POS for x in (0, 1)) +
        tuple(f"pre:{p}/x{x}" for p in PRE for x in (0, 1)))


# ---- integers and words ---------------------------------------------------------
def to_words(xs, W):
    """Keys (ints of 64 W bits) -> uint64[W][n], word 0 the most significant."""
    out = np.zeros((W, len(xs)), np.uint64)
    for j in range(W):
        sh = 64 * (W - 1 - j)
        out[j] = np.array([(x >> sh) & M64 for x in xs], np.uint64) if len(xs) else 0
    return out


def from_words(words):
    """uint64[W][n] -> list of ints."""
    words = np.asarray(words, np.uint64)
    W, n = words.shape
    out = [0] * n
    for j in range(W):
        col = words[j].tolist()
        out = [(o << 64) | c for o, c in zip(out, col)]
    return out


def randbits(rng, n):
    if n == 0:
        return 0
    return int.from_bytes(rng.bytes((n + 7) // 8), "big") >> (-n % 8)


def gather(x, V):
    """The bits of x at positions V (most significant first) as a code."""
    c = 0
    for p in V:
        c = (c << 1) | ((x >> p) & 1)
    return c


def spread(code, V):
    """The code's len(V) bits put at positions V (most significant first)."""
    x, n = 0, len(V)
    for i, p in enumerate(V):
        if (code >> (n - 1 - i)) & 1:
            x |= 1 << p
    return x


# ---- a group ----------------------------------------------------------------------
class Site:
    """A constant bit position b inside the key length: where a bound may
    leave the pattern first.  xb = the bound's bit there (the pattern's
    inverted), npb / k = varying bits above / below b."""

    def __init__(self, g, b):
        self.b, self.xb = b, 1 - ((g.C >> b) & 1)
        self.npb = sum(1 for p in g.V if p > b)
        self.k = len(g.V) - self.npb
        self.labels = g.pos_labels(b, self.npb, self.k)


class Group:
    """Rows of one group over the pattern C and the varying mask M.

    The mask leaves constant: the key's first and last byte (sites above and
    below every varying bit, with pattern bits of both values), bit 63 and bit
    0 of every word, the word `zero_word`, and whatever `bits` does not take of
    the rest (or of `universe`).  Words at or past ceil(klen / 8), and the
    bytes past klen, are zero in every row and bound."""

    def __init__(self, W, klen, bits, nrows, rng, zero_word=None, C=None, universe=None, extra=None):
        self.W, self.klen, self.nb = W, klen, 64 * W
        self.wl = (klen + 7) // 8
        low = self.nb - 8 * klen                    # the lowest bit inside the key
        self.low = low
        self.valid = ((1 << self.nb) - 1) ^ ((1 << low) - 1)
        free = [p for p in range(low + 8, self.nb - 8)
                if p % 64 not in (0, 63) and W - 1 - p // 64 != zero_word]
        if universe is not None:
            free = [p for p in free if (universe >> p) & 1]
        assert len(free) >= bits, (len(free), bits)
        pick = rng.choice(len(free), bits, replace=False) if bits else []
        self.M = sum(1 << free[i] for i in pick)
        self.V = [p for p in range(self.nb - 1, -1, -1) if (self.M >> p) & 1]
        self.bits = bits
        if C is None:
            C = randbits(rng, self.nb)
            C &= ~(0xFF << (self.nb - 8))
            C |= 0x5A << (self.nb - 8)              # first byte: 0 and 1 above every varying bit
            C &= ~(0xFF << low)
            C |= 0xA5 << low                        # last byte: 0 and 1 below every varying bit
            for j in range(W):                      # bit 63 / bit 0 of the words: both values
                for r, v in ((63, (j + 1) % 2), (0, j % 2)):
                    p = 64 * (W - 1 - j) + r
                    if low + 8 <= p < self.nb - 8:
                        C = (C & ~(1 << p)) | (v << p)
        self.C = C & self.valid & ~self.M
        self.sites = [Site(self, b) for b in range(low, self.nb) if not (self.M >> b) & 1]
        # rows
        rows = {self.C, self.C | self.M}
        singles = self.V if bits <= 190 else [self.V[i] for i in sorted(rng.choice(bits, 190, replace=False))]
        rows |= {self.C | (1 << p) for p in singles}
        self.anchor = {}
        for cls in ("carry", "borrow"):
            for xb in (0, 1):
                a = self._anchor(cls, xb, rng)
                if a is not None:
                    self.anchor[(cls, xb)] = a[:2]
                    rows.add(a[2])
        if extra is not None:
            more = extra(self)
            assert not rows & set(more)
            rows |= set(more)
        assert len(rows) <= nrows, (len(rows), nrows)
        while len(rows) < nrows:
            rows.add(self.C | (randbits(rng, self.nb) & self.M))
        self.rows = sorted(rows)
        self.rowset = rows
        acc = 0
        for r in self.rows:
            acc |= r ^ self.rows[0]
        assert acc == self.M, "the rows do not vary in exactly M"
        assert all(r & ~self.valid == 0 for r in self.rows)
        self.top = self.valid                       # the largest bound: 0xFF in every key byte

    def word_mask(self, j):
        return (self.M >> (64 * (self.W - 1 - j))) & M64

    def pos_labels(self, b, npb, k):
        j, r = self.W - 1 - b // 64, b % 64
        wm = self.word_mask(j)
        out = set()
        if npb == 0:
            out.add("np0")
        if k == 0:
            out.add("k0")
        if wm >> (r + 1) and wm & ((1 << r) - 1):
            out.add("between")
        if r == 63:
            out.add("bit63")
        if r == 0:
            out.add("bit0")
        if wm == 0:
            out.add("zero-mask-word")
        if j == self.wl - 1:
            out.add("last-word")
        return out

    def _anchor(self, cls, xb, rng):
        """A site and a prefix whose +1 carries (-1 borrows) from code word
        w >= 1 into word w - 1, and a row with that prefix: the rows next to
        the bound then show a step that stops at the word."""
        cand = [s for s in self.sites if s.xb == xb and s.k >= 1 and s.npb >= 66 and (s.npb - 1) % 64 >= 1]
        if not cand:
            return None
        s = cand[int(rng.integers(len(cand)))]
        tail = s.npb - 64 * ((s.npb - 1) // 64)
        high = randbits(rng, s.npb - tail)
        top = 1 << (s.npb - tail - 1)
        high = (high & ~top) if cls == "carry" else (high | top)   # neither all ones nor zero
        P = (high << tail) | ((1 << tail) - 1 if cls == "carry" else 0)
        row = self.C | spread(P, self.V[:s.npb]) | (randbits(rng, self.nb) & spread((1 << s.k) - 1, self.V[s.npb:]))
        return s, P, row

    # -- bounds --
    def make(self, s, prefix, lowbits):
        """The bound that agrees with the pattern above site s, holds `prefix`
        in the varying bits above it, leaves the pattern at s and holds
        `lowbits` below."""
        above = ~((1 << (s.b + 1)) - 1)
        return ((self.C & above) | spread(prefix, self.V[:s.npb]) | (s.xb << s.b) |
                (lowbits & ((1 << s.b) - 1) & self.valid))

    def _low(self, rng):
        return (0, self.valid, randbits(rng, self.nb))[int(rng.integers(3))]

    def _pick(self, cand, rng, n=2):
        if not cand:
            return []
        idx = rng.choice(len(cand), min(n, len(cand)), replace=False)
        return [cand[int(i)] for i in idx]

    def placed(self, rng):
        """[(X, tag)]: the bounds of this group, by branch."""
        out = []
        rows = self.rows
        for r in {rows[0], rows[-1], rows[int(rng.integers(len(rows)))]}:
            out.append((r, "exact-present"))
        if self.bits >= 8:
            n = 0
            while n < 2:
                x = self.C | (randbits(rng, self.nb) & self.M)
                if x not in self.rowset:
                    out.append((x, "exact-absent"))
                    n += 1
        row_prefix = lambda s: gather(rows[int(rng.integers(len(rows)))], self.V[:s.npb])
        for name in POS:
            for xb in (0, 1):
                cand = [s for s in self.sites if name in s.labels and s.xb == xb]
                for s in self._pick(cand, rng):
                    out.append((self.make(s, row_prefix(s), self._low(rng)), f"pos:{name}/x{xb}"))
        for xb in (0, 1):
            inner = [s for s in self.sites if s.xb == xb and s.npb >= 2 and s.k >= 1]
            inner = inner or [s for s in self.sites if s.xb == xb and s.npb >= 2]
            for s in self._pick(inner, rng):
                out.append((self.make(s, 0, self._low(rng)), f"pre:zeros/x{xb}"))
            for s in self._pick(inner, rng):
                out.append((self.make(s, (1 << s.npb) - 1, self._low(rng)), f"pre:ones/x{xb}"))
            for s in self._pick(inner, rng):
                for _ in range(16):
                    x = self.make(s, row_prefix(s), self._low(rng))
                    if f"pre:generic/x{xb}" in classify(x, self):
                        out.append((x, f"pre:generic/x{xb}"))
                        break
            for cls in ("carry", "borrow"):
                if (cls, xb) in self.anchor:
                    s, P = self.anchor[(cls, xb)]
                    out.append((self.make(s, P, self._low(rng)), f"pre:{cls}/x{xb}"))
        out.append((0, "zero"))
        out.append((self.top, "max"))
        return out

    def collapsing(self, rng):
        """(lo, hi): a row as lo under an off-pattern hi that leaves the
        pattern below every varying bit with a one -- hi' = lo', a range that
        takes the point index."""
        cand = [s for s in self.sites if s.k == 0 and s.xb == 1 and s.npb == self.bits]
        if not cand:
            return None
        s = cand[int(rng.integers(len(cand)))]
        row = self.rows[int(rng.integers(len(self.rows)))]
        hi = self.make(s, gather(row, self.V), self._low(rng))
        assert hi > row
        return row, hi


def classify(X, g):
    """The tags of bound X in group g, from (X, C, M) alone."""
    tags = set()
    if X == 0:
        tags.add("zero")
    if X == g.top:
        tags.add("max")
    d = (X ^ g.C) & ~g.M & ((1 << g.nb) - 1)
    if d == 0:
        tags.add("exact-present" if X in g.rowset else "exact-absent")
        return tags
    b = d.bit_length() - 1
    xb = (X >> b) & 1
    npb = sum(1 for p in g.V if p > b)
    k = len(g.V) - npb
    for name in g.pos_labels(b, npb, k):
        tags.add(f"pos:{name}/x{xb}")
    if npb:
        prefix = gather(X, g.V[:npb])
        w = (npb - 1) // 64                 # the code word of the prefix's last bit
        tail = npb - 64 * w                 # prefix bits in that word
        lowp = prefix & ((1 << tail) - 1)
        if prefix == 0:
            name = "zeros"
        elif prefix == (1 << npb) - 1:
            name = "ones"
        elif w >= 1 and lowp == (1 << tail) - 1:
            name = "carry"
        elif w >= 1 and lowp == 0:
            name = "borrow"
        else:
            name = "generic"
        tags.add(f"pre:{name}/x{xb}")
    return tags


# ---- the point index, restated to choose rows ------------------------------------------
def ph_mix(k0, k1, k2):
    h = (k0 * 0x9E3779B97F4A7C15) & M64
    h ^= ((k1 + 0x632BE59BD9B4E019) * 0xC2B2AE3D27D4EB4F) & M64
    h ^= ((k2 + 0x165667B19E3779F9) * 0xD6E8FEB86659FD93) & M64
    h ^= h >> 31
    h = (h * 0xBF58476D1CE4E5B9) & M64
    return h ^ (h >> 29)


def ph_key(gid, code, bits, WC, gb, WG):
    """The tiles' key gid || code of a `bits`-bit code (left-aligned in WC words)."""
    c = code << (64 * WC - bits)
    x = [(c >> (64 * (WC - 1 - j))) & M64 if j < WC else 0 for j in range(3)]
    if gb == 0:
        k = x
    else:
        k = [((gid << (64 - gb)) | (x[0] >> gb)) & M64,
             ((x[0] << (64 - gb)) | (x[1] >> gb)) & M64,
             ((x[1] << (64 - gb)) | (x[2] >> gb)) & M64]
    return [k[j] if j < WG else 0 for j in range(3)]


def point_home(gid, code, bits, WC, gb, WG, nrows):
    """Home bucket of a key in the point index of a window of `nrows` distinct
    rows -- ph_mix, ph_key and point_hash_buckets (nb = n + 64) of
    comdb2_amd/csrc/hsc_compact.hip restated over Python integers.  It is used
    only to choose which rows a case holds and probes; every expectation comes
    from the integer model.  If the device hash drifts from this restatement
    the placed rows no longer share a bucket: the case gets weaker, not wrong."""
    nb = nrows + 64
    return (ph_mix(*ph_key(gid, code, bits, WC, gb, WG)) * nb) >> 64


SAME_HOME, LAST_HOME = 9, 5      # rows sharing one home bucket / homed in the last bucket


def place_points(g, gid, WC, gb, WG, nrows, taken):
    """Codes of group g by home bucket: SAME_HOME + 2 with one home (the last
    two stay absent), LAST_HOME + 1 in the last bucket (the last stays absent)."""
    home = lambda c: point_home(gid, c, g.bits, WC, gb, WG, nrows)
    same, last, target = [], [], None
    c = 0
    while len(same) < SAME_HOME + 2 or len(last) < LAST_HOME + 1:
        c += 1
        assert c < 1 << g.bits
        if g.C | spread(c, g.V) in taken:
            continue
        h = home(c)
        if h == nrows + 63:
            if len(last) < LAST_HOME + 1:
                last.append(c)
        elif target is None or h == target:
            target = h
            if len(same) < SAME_HOME + 2:
                same.append(c)
    return same, last


# ---- cases ---------------------------------------------------------------------------
class Case:
    """One window and its placed probes.

    spec: W, mains [(klen, bits, nrows)], and optionally alone (no further
    group), fillers (count, bits, nrows), shared (every group on one pattern,
    its varying bits inside one 48-bit universe), zero_word of the mains.
    Further groups of every case but `alone`: one distinct key, a registered
    group without rows, a group of 9 varying bits (its code left-aligned with a
    long zero tail, its key three bytes into the last word), and the group of
    the point-index rows."""

    def __init__(self, name, spec):
        self.name, self.W = name, spec["W"]
        W = self.W
        rng = np.random.default_rng(sum(name.encode()) * 1000003 + 17)
        self.groups, self.g = [], []                 # (table, index, klen); Group or None
        shared = spec.get("shared", False)
        C = universe = None
        if shared:                                   # <= 62 varying bits over the whole window
            C = randbits(rng, 64 * W)
            uni = [p for p in range(8, 64 * W - 8) if p % 64 not in (0, 63) and W - 1 - p // 64 != 1]
            universe = sum(1 << uni[i] for i in rng.choice(len(uni), 48, replace=False))

        def add(klen, g):
            self.groups.append((f"t{len(self.groups) % 5}", len(self.groups) // 5, klen))
            self.g.append(g)
            return len(self.g) - 1

        self.mains = []
        for klen, bits, nrows in spec["mains"]:
            self.mains.append(add(klen, Group(W, klen, bits, nrows, rng, spec.get("zero_word"), C, universe)))
        self.placed_groups = list(self.mains)
        self.alone = spec.get("alone", False)
        fillers = spec.get("fillers", (0, 0, 0))
        self.pg = None
        if not self.alone:
            full = 8 * W
            self.single = add(full if shared else min(9, full), None)
            self.g[self.single] = Group(W, self.groups[self.single][2], 0, 1, rng, None, C, universe)
            self.norows = add(full, None)
            lk = full if shared else 8 * (W - 1) + 3
            self.lowbits = add(lk, Group(W, lk, 9, 40, rng, None if shared else 0, C, universe))
            self.placed_groups += [self.single, self.lowbits]
            for _ in range(fillers[0]):
                add(full, Group(W, full, fillers[1], fillers[2], rng, None, C, universe))
        ng = len(self.groups) + (0 if self.alone else 1)
        self.maxbits = max(g.bits for g in self.g if g is not None)
        self.gb = (ng - 1).bit_length()
        self.code_words = self.maxbits // 64 + 1
        wg = (self.maxbits + self.gb + 1 + 63) // 64
        self.compact = self.code_words < W and self.code_words <= 6
        self.tile_key_words = wg if self.compact and wg <= 3 else 0
        self.point_rows = None
        if not self.alone:
            PG_ROWS = 60
            n_total = sum(len(g.rows) for g in self.g if g is not None) + PG_ROWS
            gid = len(self.groups)
            placed = {}

            def extra(g):
                same, last = place_points(g, gid, self.code_words, self.gb, max(self.tile_key_words, 1),
                                          n_total, {g.C, g.C | g.M} | {g.C | (1 << p) for p in g.V})
                key = lambda c: g.C | spread(c, g.V)
                placed["same"] = [key(c) for c in same[:SAME_HOME]]
                placed["last"] = [key(c) for c in last[:LAST_HOME]]
                placed["absent"] = [key(c) for c in same[SAME_HOME:] + last[LAST_HOME:]]
                return placed["same"] + placed["last"]

            self.pg = add(8 * W, Group(W, 8 * W, 24, PG_ROWS, rng, None, C, universe, extra))
            assert not set(placed["absent"]) & self.g[self.pg].rowset
            self.point_rows = placed
        assert len(self.groups) == ng
        # rows in (group, key) order, LSNs scrambled against it
        gids, keys = [], []
        for i, g in enumerate(self.g):
            if g is not None:
                gids += [i] * len(g.rows)
                keys += g.rows
        self.n = len(keys)
        assert self.n <= 4100
        lsn = np.uint64(LSN0) + A.scramble(self.n).astype(np.uint64)
        self.rows = A.Rows(np.array(gids, np.uint32), to_words(keys, W), lsn)
        self.lsn_of = {(g, k): int(l) for g, k, l in zip(gids, keys, lsn.tolist())}
        self.oldest, self.newest = LSN0, LSN0 + self.n - 1
        self._probes(rng)

    # -- probes --
    def _add(self, g, lo, hi, snap, bound=None, role=None):
        self.P.append((g, lo, hi, snap))
        self.meta.append((bound, role))

    def _probes(self, rng):
        self.P, self.meta, self.bounds = [], [], []
        for gi in self.placed_groups:
            g = self.g[gi]
            lsn = lambda r: self.lsn_of[(gi, r)]
            for X, tag in g.placed(rng):
                bi = len(self.bounds)
                self.bounds.append((gi, X, tag))
                i, j = bisect.bisect_left(g.rows, X), bisect.bisect_right(g.rows, X)
                pred = g.rows[i - 1] if i else None
                succ = g.rows[j] if j < len(g.rows) else None
                if succ is not None:
                    self._add(gi, X, succ, lsn(succ) - 1, bi, "lo")
                    self._add(gi, X, succ, lsn(succ), bi, "lo")
                    self._add(gi, succ, X, BEFORE, bi, "hi")
                if pred is not None:
                    self._add(gi, pred, X, lsn(pred) - 1, bi, "hi")
                    self._add(gi, pred, X, lsn(pred), bi, "hi")
                    self._add(gi, X, pred, BEFORE, bi, "lo")
                if X in g.rowset:
                    self._add(gi, X, X, lsn(X) - 1, bi, "both")
                    self._add(gi, X, X, lsn(X), bi, "both")
                else:
                    self._add(gi, X, X, BEFORE, bi, "both")
                self._add(gi, X, g.top, BEFORE, bi, "lo")
                self._add(gi, 0, X, BEFORE, bi, "hi")
            col = g.collapsing(rng)
            if col is not None:
                lo, hi = col
                self._add(gi, lo, hi, lsn(lo) - 1)
                self._add(gi, lo, hi, lsn(lo))
        if not self.alone:
            top = (1 << 64 * self.W) - 1
            self._add(self.norows, 0, top, BEFORE)
            self._add(self.norows, top >> 9 << 9, top >> 9 << 9, BEFORE)
            gi, g = self.pg, self.g[self.pg]
            for r in self.point_rows["same"] + self.point_rows["last"]:
                self._add(gi, r, r, self.lsn_of[(gi, r)] - 1)
                self._add(gi, r, r, self.lsn_of[(gi, r)])
            for r in self.point_rows["absent"]:
                self._add(gi, r, r, BEFORE)
        # snapshots around one row: the oldest, the newest and another
        self.snap_from = len(self.P)
        by_lsn = {l: gk for gk, l in self.lsn_of.items()}
        for l in (self.oldest, self.newest, self.oldest + self.n // 2):
            gi, r = by_lsn[l]
            g = self.g[gi]
            i = bisect.bisect_left(g.rows, r)
            lo = g.rows[i - 1] + (1 << g.low) if i else 0    # just above the row before
            for snap in (l, l - 1, 0, self.oldest - 1, self.newest + 1, self.newest + (1 << 32), 1 << 62):
                self._add(gi, r, r, snap)
                self._add(gi, lo, r, snap)

    def order(self, name):
        """Indices into the probes (a point may come more than once)."""
        pts = [i for i, p in enumerate(self.P) if p[1] == p[2]]
        rngs = [i for i, p in enumerate(self.P) if p[1] != p[2]]
        if name == "points-first":      # whole waves of points: the ranges start a wave
            fill = [pts[i % len(pts)] for i in range(-len(pts) % 64)]
            return pts + fill + rngs
        if name == "alternating":       # a point and a range in every pair of lanes
            out = []
            for i, r in enumerate(rngs):
                out += [pts[i % len(pts)], r]
            return out
        assert name == "shuffle"
        return np.random.default_rng(len(self.P)).permutation(len(self.P)).tolist()

    @functools.lru_cache(maxsize=None)
    def batch(self, name):
        idx = self.order(name)
        P = [self.P[i] for i in idx]
        return A.batch(self.W, [p[0] for p in P], to_words([p[1] for p in P], self.W),
                       to_words([p[2] for p in P], self.W), [p[3] for p in P])

    def snapshot_batch(self):
        """The probes of the snapshots around one row alone: a point and a
        range at the row's LSN, the LSN before, 0, below the oldest commit and
        above the newest (past both clamps of the 32-bit commit ranks)."""
        P = self.P[self.snap_from:]
        return A.batch(self.W, [p[0] for p in P], to_words([p[1] for p in P], self.W),
                       to_words([p[2] for p in P], self.W), [p[3] for p in P])

    def model(self):
        return Model(self.W, self.rows)


class Model:
    """Read set t conflicts iff some row of its group has lo <= row <= hi as
    integers and lsn > snap."""

    def __init__(self, W, rows):
        self.W = W
        self.by_group = {}
        for g, k, l in zip(rows.gid.tolist(), from_words(rows.words), rows.lsn.tolist()):
            self.by_group.setdefault(g, []).append((k, l))
        for v in self.by_group.values():
            v.sort()

    def verdicts(self, m):
        assert m["words"] == self.W and m["n_lock"] == 0
        out = np.zeros(m["n_txn"], bool)
        lo, hi = from_words(m["lo"]), from_words(m["hi"])
        for q in range(m["n"]):
            rows = self.by_group.get(int(m["gid"][q]), [])
            s = int(m["snap"][q])
            if any(lo[q] <= k <= hi[q] and l > s for k, l in rows):
                out[int(m["txn"][q])] = True
        return out


# (W, maxbits) -> code words; the tile key takes ceil((maxbits + group bits + 1) / 64) words
SPECS = {
    "w2-63": dict(W=2, mains=[(16, 63, 160)]),
    "w3-64": dict(W=3, mains=[(24, 64, 160)]),
    "w3-127": dict(W=3, mains=[(24, 127, 300)], fillers=(8, 40, 250)),     # 2401 rows: two tiles
    "w4-128": dict(W=4, mains=[(30, 128, 300)]),
    "w8-191-one": dict(W=8, mains=[(58, 191, 300)], alone=True, zero_word=3),
    "w8-191": dict(W=8, mains=[(58, 191, 300)]),
    "w8-192": dict(W=8, mains=[(64, 192, 300)]),
    "w8-383": dict(W=8, mains=[(64, 383, 300)]),
    "w8-384": dict(W=8, mains=[(64, 384, 300)]),
    "w9-100": dict(W=9, mains=[(72, 100, 200)]),
    "w3-62": dict(W=3, mains=[(24, 48, 120)], shared=True),
    "w8-many": dict(W=8, mains=[(64, 120, 200), (40, 90, 150)], fillers=(88, 20, 40)),  # 94 groups
}
# expected (code_words, tile_key_words); code_words None: the window is not compact
EXPECT = {
    "w2-63": (1, 2), "w3-64": (2, 2), "w3-127": (2, 3), "w4-128": (3, 3), "w8-191-one": (3, 3),
    "w8-191": (3, 0), "w8-192": (4, 0), "w8-383": (6, 0), "w8-384": (None, 0), "w9-100": (2, 2),
    "w3-62": (1, 1), "w8-many": (2, 2),
}
NAMES = tuple(SPECS)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name, SPECS[name])


# ---- rebuilds of the point index --------------------------------------------------------
class RebuildCase:
    """Two windows of equal row count and disjoint keys over the same groups,
    patterns and masks (a key has the same code in both): ingested one after
    the other into one context, the point buffer is reused at the next epoch
    and still holds the other window's keys.  Probes: a point on every row of
    both windows -- its own rows at the LSN before theirs (a conflict) and at
    their LSN, the other window's before every row."""

    W = 3
    GROUPS = [("t0", 0, 24), ("t1", 0, 24)]
    BITS, NROWS = (70, 30), 150

    def __init__(self):
        rng = np.random.default_rng(77)
        base = [Group(self.W, 24, b, self.NROWS, rng) for b in self.BITS]
        self.windows = []
        seen = [set(), set()]
        for w in range(2):
            gids, keys = [], []
            for gi, g in enumerate(base):
                mine = set()
                while len(mine) < self.NROWS:
                    r = g.C | (randbits(rng, g.nb) & g.M)
                    if r not in seen[gi]:
                        mine.add(r)
                        seen[gi].add(r)
                acc = 0
                for r in mine:
                    acc |= r ^ min(mine)
                assert acc == g.M
                gids += [gi] * self.NROWS
                keys += sorted(mine)
            n = len(keys)
            lsn = np.uint64(LSN0 + 1000 * w) + A.scramble(n)[::-1 if w else 1].astype(np.uint64)
            self.windows.append((A.Rows(np.array(gids, np.uint32), to_words(keys, self.W), lsn), gids, keys))
        assert len(self.windows[0][0]) == len(self.windows[1][0])
        self.code_words, self.tile_key_words = 2, 2

    def rows(self, w):
        return self.windows[w][0]

    def batch(self, w):
        """The probes while window w is ingested."""
        own, gids, keys = self.windows[w]
        _, ogids, okeys = self.windows[1 - w]
        l = own.lsn.tolist()
        g = gids + gids + ogids
        k = keys + keys + okeys
        snap = [x - 1 for x in l] + l + [BEFORE] * len(okeys)
        o = np.random.default_rng(w).permutation(len(g))
        kw = to_words([k[i] for i in o], self.W)
        return A.batch(self.W, [g[i] for i in o], kw, kw, [snap[i] for i in o])


@functools.lru_cache(maxsize=None)
def rebuild_case():
    return RebuildCase()
