"""The selectv known answers (tests/golden/selectv_range.json) embedded in
filler that cannot change a verdict by construction, for the probe paths whose
behaviour changes with the window's and the batch's size.

A *window* is the log as it stands at one checked commit of one scenario
variant, with:
  * filler commits of two tables no scenario range names, A_FILL and Z_FILL,
    whose key groups are registered before and after t1's (groups sort by id
    in the window, ids are given in registration order: register_groups) --
    A_FILL holds exactly `offset` rows, all committed before the scenario's
    first event, so the scenario's first window row is row `offset`; Z_FILL
    holds T + 37 rows from before the scenario's first event and 32 more per
    checked commit, committed between that txn's snapshot and its commit;
  * a pool of 129 read sets: the scenario txn's own (index 0, the
    reference's verdict) and 128 decoys with verdicts known by construction
    -- a *pass* decoy is a point range on a filler key that nothing wrote
    after the decoy's snapshot (an early key at the txn's snapshot, or one of
    the 32 late keys at a snapshot taken after them), a *fail* decoy a point
    range on one of the 32 late keys at the txn's snapshot.
Batches of the sizes where the 64-bit verdict words change are cut from the
pool with the scenario's read set first, last and at index 63 / 64.

Every passing scenario commit and every autocommit write is logged, so a later
commit of the scenario sees what the reference's did; what a scenario commit
does is taken from reference_commits, not from any checker."""
import copy

import numpy as np

from comdb2_amd import formats as F
from comdb2_amd.formats import LogBuilder, Range, ReadSets
from comdb2_amd.workloads import commit_checked
from helpers import selectv_cases, selectv_events

A_FILL, Z_FILL = "a_fill", "z_fill"
TABLES = [A_FILL, "t1", "t2", Z_FILL]
PER_COMMIT = 64           # filler keys per early filler commit
LATE = (2, 16)            # late filler: commits x keys, per checked commit
Z_EXTRA = 37              # Z_FILL's early rows past a tile
POOL = 129
# (batch size, positions of the scenario's read set)
BATCHES = [(1, (0,)), (63, (0, 62)), (64, (0, 63)), (65, (0, 63, 64)), (129, (0, 63, 64, 128))]


def filler_key(kind, j):
    """kind "narrow": one int64 field -- with t1's 5-byte keys the window still
    fits the 62-bit codes of the narrow layout.  kind "wide": two int64 fields,
    the first spread over all 64 bits, so the window does not fit them."""
    if kind == "narrow":
        return F.enc_int64(j)
    spread = ((j * 0x9E3779B97F4A7C15 + 0x1234567) & ((1 << 64) - 1)) - (1 << 63)
    return F.enc_int64(spread) + F.enc_int64(j)


def key_len(kind):
    return len(filler_key(kind, 0))


def register_groups(v, kind):
    """Fix the window's group order on a fresh context: A_FILL < t1 < Z_FILL.
    -> (gid of A_FILL, gid of t1, gid of Z_FILL)"""
    g = (v.register_group(A_FILL, 0, key_len(kind)), v.register_group("t1", 0, 5),
         v.register_group(Z_FILL, 0, key_len(kind)))
    assert g[0] < g[1] < g[2]
    return g


def _fill(lb, tb, kind, j0, n, per_commit):
    for c in range(j0, j0 + n, per_commit):
        name = ("fill", tb, c)
        lb.begin(name)
        for j in range(c, min(c + per_commit, j0 + n)):
            lb.write(name, F.REC_UNDO_ADD_IX, tb, 0, filler_key(kind, j))
        lb.commit(name)


class Window:
    """log, pool (ReadSets of POOL read sets), want (bool[POOL], by
    construction; want[0] is the reference's verdict) and what it is."""

    def __init__(self, what, log, pool, want):
        self.what, self.log, self.pool, self.want = what, log, pool, want

    def batches(self):
        """-> [((size, position), read-set indices into the pool)]"""
        out = []
        for n, positions in BATCHES:
            for p in positions:
                decoys = list(range(1, n))
                out.append(((n, p), decoys[:p] + [0] + decoys[p:]))
        return out


def build(T, kind, offsets=None, z_early=None):
    """-> [Window] for every checked commit of every scenario variant at every
    offset of the scenario's first row (default 0, T - 1 and T)."""
    offsets = (0, T - 1, T) if offsets is None else offsets
    z_early = T + Z_EXTRA if z_early is None else z_early
    out = []
    for offset in offsets:
        base = LogBuilder(TABLES)
        _fill(base, A_FILL, kind, 0, offset, PER_COMMIT)
        _fill(base, Z_FILL, kind, 0, z_early, PER_COMMIT)
        for name, vname, sc in selectv_cases():
            lb = copy.deepcopy(base)
            verdict = dict(zip(sc["commits"], sc["reference_commits"]))
            snaps, z_next = {}, z_early
            for ev, t in selectv_events(sc):
                if ev == "begin":
                    snaps[t.name] = lb.next_lsn()
                    continue
                if t.name in verdict and commit_checked(t):
                    late = list(range(z_next, z_next + LATE[0] * LATE[1]))
                    _fill(lb, Z_FILL, kind, z_next, len(late), LATE[1])
                    z_next += len(late)
                    out.append(_window(f"{name}-{vname} offset {offset} commit {t.name}", lb, kind, t,
                                       snaps[t.name], verdict[t.name], offset, z_early, late))
                if t.writes and not verdict.get(t.name, 0):
                    lb.begin(t.name)
                    for rt, tb, ix, key in t.writes:
                        lb.write(t.name, rt, tb, ix, key)
                    lb.commit(t.name)
    return out


def _window(what, lb, kind, t, snap, verdict, n_a, z_early, late):
    after = lb.next_lsn()  # nothing is logged past this yet: a snapshot at the end of the log
    sets, snaps, want = [list(t.reads)], [snap], [bool(verdict)]
    for d in range(1, POOL):
        if d % 3 == 0:                           # fail: a late key, the txn's snapshot
            tb, j, s, w = Z_FILL, late[d % len(late)], snap, True
        elif d % 3 == 1:                         # pass: an early key, the txn's snapshot
            tb, j = (A_FILL, (d * 7) % n_a) if n_a and d % 2 else (Z_FILL, (d * 11) % z_early)
            s, w = snap, False
        else:                                    # pass: a late key, a snapshot after it
            tb, j, s, w = Z_FILL, late[d % len(late)], after, False
        k = filler_key(kind, j)
        sets.append([Range(tb, 0, k, k)])
        snaps.append(s)
        want.append(w)
    log = lb.build()
    return Window(what, log, ReadSets.from_lists(sets, snaps, tbnames=log.tbnames), np.array(want))
