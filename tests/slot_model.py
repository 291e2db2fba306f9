"""A numpy model of the narrow tiles' slot tables (k_recent) and of the
records the fast locate instances drop by them (k_locate_t,
comdb2_amd/csrc/hsc_narrow.hip).

A window is one index of distinct int64 keys in key order with a commit LSN
each.  Codes are (key - first key) >> tz, tz = the low bits every key shares;
tile t holds rows 4096 t .. and starts at code first[t].  Per tile:

  span    first[t + 1] - first[t], clamped to 2^32; 2^32 for the last tile
  shift   the least s with (span - 1) >> s < 512
  slot    of a row: min(key32 >> shift, 511), key32 = code - first[t]
  table   [512] u16: max(rank32) >> qshift over the slot's rows, 0 if none

rank32 = LSN - oldest LSN + 1 (the window's LSNs span < 2^32 - 2), r(S) the
same map of a snapshot clamped to [0, 2^32 - 1], and qshift the least q with
(largest rank32) >> q < 65536.  A window of a wider LSN span ranks by the
index among its distinct LSNs and takes a general locate instance, which
drops nothing (`filters` is False).

The locate's end-tile step gives a range [lo, hi] a record {tile, lo32, hi32,
r(S)} in each end tile it covers partly (`records`; a fully covered tile is
answered by the tile maxima and leaves none).  A record is dropped when its
bounds reach at most two adjacent slots, min(hi32 >> shift, 511) -
min(lo32 >> shift, 511) <= 1, and both slots' entries are < r(S) >> qshift.
The slot map is monotone, so every row inside the bounds lies in one of the
two slots, and entry < r(S) >> qshift implies rank32 < r(S) for each of them:
no row the conflict test rank32 > r(S) could accept.
"""

import numpy as np

TILE = 4096
SLOTS_LOG2 = 9
SLOTS = 1 << SLOTS_LOG2
U32 = 0xFFFFFFFF
LSN32_MAX_SPAN = 0xFFFFFFFD


def slot_shift(span):
    """The least s with (span - 1) >> s < 512; span in [1, 2^32]."""
    bits = int(min(max(int(span), 1), 1 << 32) - 1).bit_length()
    return max(bits - SLOTS_LOG2, 0)


def qshift_of(max_rank):
    q = 0
    while (int(max_rank) >> q) >= 65536:
        q += 1
    return q


class SlotWindow:
    def __init__(self, keys, lsn, qshift=None):
        """qshift: None = derived from the window (what the library does); a
        value = the table at that quantum (the model's own tests: any q for
        which the entries fit a u16 is sound)."""
        keys = np.asarray(keys, np.int64)
        lsn = np.asarray(lsn, np.uint64)
        assert len(keys) and len(keys) == len(lsn) and (np.diff(keys) > 0).all()
        self.keys, self.lsn = keys, lsn
        d = (keys - keys[0]).astype(np.uint64)
        orv = int(np.bitwise_or.reduce(d))
        self.tz = (orv & -orv).bit_length() - 1 if orv else 0
        self.code = d >> np.uint64(self.tz)
        self.ntiles = (len(keys) + TILE - 1) // TILE
        self.first = self.code[::TILE].copy()
        self.base = int(lsn.min())
        self.filters = int(lsn.max()) - self.base <= LSN32_MAX_SPAN
        if self.filters:
            self.rank = (lsn - np.uint64(self.base) + np.uint64(1)).astype(np.int64)
        else:
            self.commits = np.unique(lsn)
            self.rank = 1 + np.searchsorted(self.commits, lsn).astype(np.int64)
        self.qshift = qshift_of(self.rank.max()) if qshift is None else qshift
        assert (int(self.rank.max()) >> self.qshift) < 65536
        span = np.full(self.ntiles, 1 << 32, np.int64)
        span[:-1] = np.minimum(np.diff(self.first.astype(np.int64)), 1 << 32)
        self.shift = np.array([slot_shift(s) for s in span], np.int64)
        tile = np.arange(len(keys)) // TILE
        self.key32 = (self.code - self.first[tile]).astype(np.int64)
        assert self.key32.max() <= U32
        self.slot = np.minimum(self.key32 >> self.shift[tile], SLOTS - 1)
        smax = np.zeros((self.ntiles, SLOTS), np.int64)
        np.maximum.at(smax, (tile, self.slot), self.rank)
        self.smax = smax  # exact, before the quantum
        self.table = smax >> self.qshift

    def snap_rank(self, snap):
        snap = np.asarray(snap, np.uint64)
        if not self.filters:
            return np.searchsorted(self.commits, snap, side="right").astype(np.int64)
        d = np.where(snap < np.uint64(self.base), 0,
                     np.minimum(snap - np.uint64(self.base), np.uint64(U32 - 1)).astype(np.int64) + 1)
        return np.minimum(d, U32).astype(np.int64)

    def bound_codes(self, lo, hi):
        """lo -> ceil((lo - key0) / 2^tz), 0 below the window; hi -> floor,
        live = False below the window.  Python ints / int64, no overflow for
        the bounds the tests use (|bound - key0| < 2^63)."""
        lo = np.asarray(lo, np.int64) - self.keys[0]
        hi = np.asarray(hi, np.int64) - self.keys[0]
        unit = np.int64(1) << np.int64(self.tz)
        clo = np.where(lo <= 0, 0, (np.maximum(lo, 0) + (unit - 1)) >> np.int64(self.tz))
        live = hi >= 0
        chi = np.where(live, np.maximum(hi, 0) >> np.int64(self.tz), 0)
        return clo.astype(np.int64), chi.astype(np.int64), live

    def records(self, lo, hi, snap):
        """The join records the end-tile step locates for ranges [lo, hi]
        (int64 key values) at snapshots `snap`: arrays (probe, tile, lo32,
        hi32, rs), a range's first-tile record before its last-tile one."""
        clo, chi, live = self.bound_codes(lo, hi)
        rs = self.snap_rank(snap)
        first = self.first.astype(np.int64)
        ok = live & (clo <= chi)
        ca = np.searchsorted(first, clo, side="left")    # #first < lo
        cb = np.searchsorted(first, chi, side="right")   # #first <= hi
        a = np.maximum(ca - 1, 0)
        bt = np.maximum(cb - 1, 0)
        ok &= (cb > 0) & (a <= bt)
        fa, fb = first[a], first[bt]
        lo_a = np.maximum(clo - fa, 0)
        none = np.int64(-1)
        hi_a = np.where(a == bt, np.where(chi < fa, none, chi - fa), U32)
        hi_b = np.where(chi < fb, none, chi - fb)
        full_a = (lo_a == 0) & ((a < bt) | (hi_a >= U32))
        use_a = (lo_a <= U32) & (hi_a != none) & (lo_a <= hi_a)
        use_b = (a < bt) & (hi_b != none)
        full_b = hi_b >= U32
        rec_a = ok & use_a & ~full_a
        rec_b = ok & use_b & ~full_b
        ia, ib = np.flatnonzero(rec_a), np.flatnonzero(rec_b)
        probe = np.concatenate([ia, ib])
        tile = np.concatenate([a[ia], bt[ib]])
        l32 = np.concatenate([lo_a[ia], np.zeros(len(ib), np.int64)])
        h32 = np.concatenate([np.minimum(hi_a[ia], U32), hi_b[ib]])
        o = np.argsort(probe, kind="stable")
        return probe[o], tile[o], l32[o], h32[o], rs[probe[o]]

    def dropped(self, tile, l32, h32, rs):
        """The drop rule per record (all False for a window that does not filter)."""
        if not self.filters:
            return np.zeros(len(tile), bool)
        sh = self.shift[tile]
        s0 = np.minimum(l32 >> sh, SLOTS - 1)
        s1 = np.minimum(h32 >> sh, SLOTS - 1)
        qr = rs >> self.qshift
        near = s1 - s0 <= 1
        s1 = np.where(near, s1, s0)
        return near & (self.table[tile, s0] < qr) & (self.table[tile, s1] < qr)

    def kept(self, lo, hi, snap):
        """(located, kept) record counts of a batch."""
        _, tile, l32, h32, rs = self.records(lo, hi, snap)
        return len(tile), int((~self.dropped(tile, l32, h32, rs)).sum())

    def newer_row_inside(self, tile, l32, h32, rs):
        """By brute force per record: a row of the tile with lo32 <= key32 <=
        hi32 and rank32 > rs."""
        out = np.zeros(len(tile), bool)
        for i in range(len(tile)):
            a, b = tile[i] * TILE, min((tile[i] + 1) * TILE, len(self.keys))
            k, r = self.key32[a:b], self.rank[a:b]
            out[i] = bool(((k >= l32[i]) & (k <= h32[i]) & (r > rs[i])).any())
        return out
