"""Hand-built histories for the dependency graph's read-search paths, and a
numpy restatement of what graph_build (comdb2_amd/csrc/hsc_graph.hip) decides
from a history's writers, so every case can assert which branch it reaches.

plan_of mirrors the build's constants: kPer = 8 writers per directory bucket,
kDMax = 23 directory bits, kPtE = 12 offsets in a bucket line and the 31-bit
offset limit of a line.  If one of them changes, the preconditions below fail
and name the case to rebuild.

cases(): name -> Case(history, expected plan fields, tags).  The tags name the
branch a case exists for (test_graph_cases.check_preconditions asserts each of
them on the CPU)."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from comdb2_amd.workloads import History

K_PER, K_DMAX, K_PT_E, K_PT_SHIFT_MAX = 8, 23, 12, 31
M64 = (1 << 64) - 1


def _popcount(x):
    return bin(int(x)).count("1")


def _compress(v, mask):
    """The bits of v under mask, packed to the low end (pext), per element."""
    v = np.asarray(v, np.uint64)
    out = np.zeros(v.shape, np.uint64)
    j = 0
    for b in range(64):
        if (int(mask) >> b) & 1:
            out |= ((v >> np.uint64(b)) & np.uint64(1)) << np.uint64(j)
            j += 1
    return out


@dataclass
class Plan:
    nw: int = 0              # write ops
    nu: int = 0              # distinct (key, txn) writers
    km: int = 0              # varying / constant bits of the writers' keys and txns
    kc: int = 0
    tm: int = 0
    tc: int = 0
    tb: int = 0              # popcount(tm)
    B: int = 0               # popcount(km) + popcount(tm): the sort's key bits
    packs: bool = False
    pk: np.ndarray = None    # the sorted distinct packed writers
    D: int = 0
    shift: int = 0
    path: str = "rows"       # pt (bucket lines) | pk (directory + packed keys) | rows
    occupancy: np.ndarray = None        # writers per directory bucket
    compressible: np.ndarray = None     # per op: a read whose observed id fits the writers' txn bits
    txn_sorted: bool = True
    sort_passes: int = 0     # 8-bit passes of a device build's writer sort


def plan_of(h) -> Plan:
    p = Plan()
    w = np.asarray(h.is_write) != 0
    key = np.asarray(h.key, np.uint64)
    txn = np.asarray(h.txn, np.uint32)
    obs = np.asarray(h.observed, np.int64)
    p.txn_sorted = bool((np.diff(txn.astype(np.int64)) >= 0).all())
    p.nw = int(w.sum())
    p.compressible = ~w
    if p.nw == 0:
        return p  # no writers: the row search over zero rows
    wk, wt = key[w], txn[w].astype(np.uint64)
    ko, ka = int(np.bitwise_or.reduce(wk)), int(np.bitwise_and.reduce(wk))
    to, ta = int(np.bitwise_or.reduce(wt)), int(np.bitwise_and.reduce(wt))
    p.km, p.tm = ko & ~ka & M64, to & ~ta & M64
    p.kc, p.tc = ka & ~p.km & M64, ta & ~p.tm & M64
    p.tb = _popcount(p.tm)
    p.B = _popcount(p.km) + p.tb
    p.packs = p.B <= 64
    p.nu = len(np.unique(np.stack([wk, wt], 1), axis=0))
    p.compressible = ~w & ((obs < 0) | ((obs & ~np.int64(p.tm)) == np.int64(p.tc)))
    if not p.packs:
        return p
    kp = _compress(wk, p.km)
    pk = ((kp << np.uint64(p.tb)) if p.tb < 64 else np.zeros_like(kp)) | _compress(wt, p.tm)
    p.pk = np.unique(pk)
    assert len(p.pk) == p.nu
    skip = p.tb if (p.txn_sorted and p.tb) else 0
    p.sort_passes = (p.B - skip + 7) // 8
    p.D = 1
    while p.D < K_DMAX and (K_PER << p.D) < p.nu:
        p.D += 1
    base, last = int(p.pk[0]), int(p.pk[-1])
    while p.shift < 64 and ((last - base) >> p.shift) >= (1 << p.D):
        p.shift += 1
    p.path = "pt" if p.shift <= K_PT_SHIFT_MAX else "pk"
    b = ((p.pk - np.uint64(base)) >> np.uint64(p.shift)) if p.shift < 64 else np.zeros(p.nu, np.uint64)
    p.occupancy = np.bincount(b.astype(np.int64), minlength=(1 << p.D) + 1)
    return p


@dataclass
class Case:
    h: History
    expect: dict = field(default_factory=dict)  # Plan fields that must equal
    tags: tuple = ()


def hist(rows, ntxn):
    """rows: (txn, key, 'r'|'w', observed writer or -1), in op order."""
    if not rows:
        return History(np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint8),
                       np.zeros(0, np.int64), ntxn)
    t, k, w, o = zip(*rows)
    return History(np.array(t, np.uint32), np.array(k, np.uint64),
                   np.array([x == "w" for x in w], np.uint8), np.array(o, np.int64), ntxn)


# ---- any_observed: arbitrary observed ids over writers with constant bits ----
KEY_CONST = (1 << 63) | (1 << 5)   # set in every key
KEY_FLIP = 1 << 40                 # clear in every writer's key: a read with it set matches no writer
_KEY_BITS = {12: list(range(8, 20)),
             45: list(range(6, 40)) + list(range(41, 52)),
             64: [b for b in range(64) if b not in (5, 40, 63)]}


def _key_values(bits, n=50):
    """n distinct keys: random values over the width's bit positions, | KEY_CONST."""
    pos = _KEY_BITS[bits]
    rng = np.random.default_rng(1000 + bits)
    while True:
        raw = rng.integers(0, 1 << 62, size=n, dtype=np.uint64) if len(pos) > 61 else \
            rng.integers(0, 1 << len(pos), size=n, dtype=np.uint64)
        vals = np.zeros(n, np.uint64)
        for j, b in enumerate(pos):
            vals |= ((raw >> np.uint64(j)) & np.uint64(1)) << np.uint64(b)
        vary = int(np.bitwise_or.reduce(vals)) & ~int(np.bitwise_and.reduce(vals))
        if len(np.unique(vals)) == n and _popcount(vary) == len(pos):
            return vals | np.uint64(KEY_CONST)


def any_observed(bits, nops=6000, seed=7):
    """4096 txns, ops in txn order; writes only by txns [1024, 2048) (their
    ids vary in 10 bits, bit 10 is constant), over 50 keys that all carry
    KEY_CONST.  Reads observe anything the ABI takes: the initial version, any
    txn id at all (mostly outside the writers' bits, below and above them), a
    real writer of the key (earlier or later than the reader), the reader
    itself, the key's last version; a tenth read a key no writer can match."""
    rng = np.random.default_rng(seed)
    ntxn = 4096
    keys = _key_values(bits)
    # a third of the ops inside the writers' txn range, the rest anywhere
    txn = np.where(rng.random(nops) < 0.3, rng.integers(1024, 2048, size=nops), rng.integers(0, ntxn, size=nops))
    txn = np.sort(txn).astype(np.uint32)
    ki = rng.integers(0, len(keys), size=nops)
    isw = ((txn >= 1024) & (txn < 2048) & (rng.random(nops) < 0.55)).astype(np.uint8)
    writers = {}
    for t, k, w in zip(txn.tolist(), ki.tolist(), isw.tolist()):
        if w:
            writers.setdefault(k, []).append(t)
    obs = np.full(nops, -1, np.int64)
    kind = rng.random(nops)
    pick = rng.random(nops)
    for i in range(nops):
        if isw[i]:
            continue
        ws = writers.get(int(ki[i]), [])
        if kind[i] < 0.15:
            continue                                   # the initial version
        if kind[i] < 0.50 or not ws:
            obs[i] = int(pick[i] * ntxn)               # any id
        elif kind[i] < 0.80:
            obs[i] = ws[int(pick[i] * len(ws))]        # a writer of the key
        elif kind[i] < 0.90:
            obs[i] = int(txn[i])                       # its own txn
        else:
            obs[i] = max(ws)                           # the last version
    key = keys[ki]
    flip = (isw == 0) & (rng.random(nops) < 0.1)
    key = np.where(flip, key ^ np.uint64(KEY_FLIP), key)
    return History(txn, key, isw, obs, ntxn)


_ANY_TAGS = ("tc", "kc", "slow_1000", "ob_self", "ob_later", "ob_last", "key_outside", "types7", "cycle")


# ---- bucket_12_13: the bucket line's capacity ----
def bucket_12_13(offset=0, lead=0, extra_obs=(), ntxn=None, readers=None, solo_at=None):
    """One key; writers lead + offset + {0..11} and lead + offset + {1000..1012}:
    D = 2, shift = 8, one bucket of exactly 12 writers (the line holds them) and
    one of 13 (the overflow search).  Every reader reads the key once per
    observed value: before, inside, at the last entry of and past each bucket.
    solo_at: instead, observed value j is read once, by txn solo_at + j alone (a
    reader of every value merges the rows of the values that share an answer,
    and a wrong one among them would hide behind the others)."""
    wr = [offset + lead + x for x in list(range(12)) + list(range(1000, 1013))]
    n = ntxn if ntxn is not None else max(wr) + 1
    # (10 and 1011: the next writer is the bucket's last entry, the 12th / 13th)
    obs = [-1] + [offset + lead + x for x in (0, 5, 10, 11, 12, 999, 1000, 1006, 1011, 1012)] + list(extra_obs)
    rows = []
    ws = set(wr)
    if solo_at is not None:
        rows = [(t, 77, "w", -1) for t in wr] + [(solo_at + j, 77, "r", o) for j, o in enumerate(obs)]
        return hist(rows, ntxn if ntxn is not None else solo_at + len(obs))
    for t in (readers if readers is not None else range(n)):
        if t in ws:
            rows.append((t, 77, "w", -1))
        rows += [(t, 77, "r", o) for o in obs]
    for t in sorted(ws - set(readers if readers is not None else range(n))):
        rows.append((t, 77, "w", -1))
    rows.sort(key=lambda r: r[0])  # (stable: a txn's ops keep their order)
    return hist(rows, n)


# ---- op-count edges of the place pass ----
def place_case(nops):
    """nops ops in txn order over 40 keys, writers at the first and last op of
    the first 4096-op block, at the first op after it and at the last op."""
    rng = np.random.default_rng(nops)
    ntxn = nops // 3 + 2
    txn = np.sort(rng.integers(0, ntxn, size=nops)).astype(np.uint32)
    key = rng.integers(0, 40, size=nops, dtype=np.uint64) * np.uint64(3) + np.uint64(1 << 33)
    isw = (rng.random(nops) < 0.4).astype(np.uint8)
    for i in (0, 4095, 4096, nops - 1):
        if i < nops:
            isw[i] = 1
    obs = np.where(rng.random(nops) < 0.3, -1, rng.integers(0, ntxn, size=nops)).astype(np.int64)
    obs[isw != 0] = -1
    return History(txn, key, isw, obs, ntxn)


PLACE_NOPS = (1, 63, 64, 65, 4095, 4096, 4097, 8193)


def _reads(key, readers, observed):
    return [(t, key, "r", o) for t in readers for o in observed]


def _sorted(rows):
    return sorted(rows, key=lambda r: r[0])


def _permuted(h, seed):
    p = np.random.default_rng(seed).permutation(len(h.txn))
    return History(h.txn[p], h.key[p], h.is_write[p], h.observed[p], h.ntxn)


@lru_cache(maxsize=None)
def cases():
    c = {}
    for bits, path in ((12, "pt"), (45, "pk"), (64, "rows")):
        c[f"any_observed[{bits}]"] = Case(any_observed(bits), dict(path=path, tm=1023, tc=1024), _ANY_TAGS)
    c["unsorted"] = Case(_permuted(any_observed(12), 3), dict(path="pt", txn_sorted=False, tm=1023, tc=1024),
                         _ANY_TAGS + ("all_passes",))
    c["bucket_12_13"] = Case(bucket_12_13(), dict(path="pt", D=2, shift=8, nu=25, km=0, tm=1023, tc=0),
                             ("bucket_12", "bucket_13"))
    # every id + 4096 + 2: a constant txn bit, the first writer above packed 0
    # (an observed 4096 compresses to x < base), observed ids past the last
    # writer (compressible: 5116, 5119; not: 5500) and below the bits (5)
    c["bucket_12_13_offset"] = Case(
        bucket_12_13(offset=4096, lead=2, extra_obs=(4096, 4097, 5116, 5119, 5, 5500), ntxn=5600,
                     readers=[0, 1, 5] + list(range(4090, 5130)) + [5500, 5599]),
        dict(path="pt", D=2, shift=8, nu=25, km=0, tm=1023, tc=4096),
        ("bucket_12", "bucket_13", "tc", "x_below_base", "x_above_last", "slow"))
    c["bucket_12_13_solo"] = Case(bucket_12_13(solo_at=1013), c["bucket_12_13"].expect, ("bucket_12", "bucket_13"))
    c["bucket_12_13_offset_solo"] = Case(
        bucket_12_13(offset=4096, lead=2, extra_obs=(4096, 4097, 5116, 5119, 5, 5500), ntxn=5600, solo_at=5200),
        c["bucket_12_13_offset"].expect, c["bucket_12_13_offset"].tags)
    c["empty_0"] = Case(hist([], 0), dict(path="rows", nw=0))
    c["empty_5"] = Case(hist([], 5), dict(path="rows", nw=0))
    c["reads_only"] = Case(hist(_sorted(_reads(9, range(6), (-1, 0, 3, 5)) + _reads(1 << 50, (2, 4), (-1, 4))), 6),
                           dict(path="rows", nw=0))
    c["writes_only"] = Case(hist(_sorted([(t, k, "w", -1) for t in range(40) for k in (t % 3, 100 + t % 7)]), 40),
                            dict(path="pt"))
    # one writer, every search outcome around it: nu = 1, base = last
    one = [(4, 8, "w", -1)]
    # (txns 8..15 read one observed value each: their rows merge with no other's)
    probes = _reads(8, range(8), (-1, 0, 3, 4, 5, 7)) + _reads(9, (1, 6), (-1, 4)) + \
        [(8 + j, 8, "r", o) for j, o in enumerate((-1, 0, 3, 4, 5, 7, 15, 8))]
    c["one_write"] = Case(hist(_sorted(one + probes), 16),
                          dict(path="pt", nu=1, B=0, D=1, shift=0, km=0, tm=0, tb=0, kc=8, tc=4), ("slow",))
    c["same_write_x3"] = Case(hist(_sorted(one * 3 + probes), 16),
                              dict(path="pt", nw=3, nu=1, B=0, D=1, shift=0, km=0, tm=0, tb=0, kc=8, tc=4),
                              ("slow",))
    # one key written by 3000 txns: km = 0 (a txn-sorted device build sorts in
    # zero passes), the unpack's 2048-row tile ends inside the key's run
    hot = [(t, 5, "w", -1) for t in range(3000)] + _reads(5, range(0, 3000, 7), (-1, 0, 2047, 2048, 2999)) + \
        [(t, 5, "r", t) for t in range(0, 3000, 11)]
    c["one_key_3000"] = Case(hist(_sorted(hot), 3000), dict(path="pt", km=0, kc=5, nu=3000, sort_passes=0),
                             ("tile_2048",))
    # one txn writing 300 keys: tm = 0, tb = 0
    wide = [(9, 1000 + 3 * k, "w", -1) for k in range(300)] + \
        [(t, 1000 + 3 * k, "r", o) for t in (2, 9, 15) for k in range(0, 300, 5) for o in (-1, 9, 3, 12)] + \
        [(3 + t % 5, 1000 + 3 * k, "r", (-1, 9, 3, 12)[k % 4]) for t in range(4) for k in range(1 + t, 300, 5)] + \
        _reads(1001, (2, 15), (-1, 9))
    c["one_txn_300_keys"] = Case(hist(_sorted(wide), 16), dict(path="pt", tm=0, tb=0, tc=9, nu=300), ("slow",))
    c["self_rmw"] = Case(hist([(0, 3, "w", -1), (1, 3, "r", 0), (1, 3, "w", -1), (1, 3, "r", 1),
                               (2, 3, "r", 2), (2, 3, "w", -1), (2, 3, "r", 2), (3, 3, "r", 1)], 4),
                         dict(path="pt", km=0), ("ob_self",))
    # duplicate read ops (duplicate raw rows), and pairs joined by two kinds of
    # edge: (1, 2) is ww on key 2 and rw on key 1; (0, 1) is ww, wr and rw on key 1
    dup = [(0, 1, "w", -1)] + [(1, 1, "r", 0)] * 3 + [(1, 1, "r", -1)] * 2 + [(1, 1, "w", -1), (1, 2, "w", -1)] + \
        [(1, 1, "r", 1)] * 2 + [(2, 1, "w", -1), (2, 2, "w", -1)] + [(2, 1, "r", 0)] * 3
    c["dup_reads"] = Case(hist(dup, 3), dict(path="pt"), ("types7", "merged_types"))
    # txn ids with long gaps, unused ids at the end (CSR offsets over empty nodes)
    gap = [(3, 1, "w", -1), (3, 2, "r", -1), (500, 1, "r", 3), (500, 2, "w", -1), (501, 1, "w", -1),
           (501, 2, "r", 70000), (501, 2, "w", -1), (70000, 2, "w", -1), (70000, 1, "r", 3)]
    c["gaps"] = Case(hist(gap, 100000), dict(path="pt"), ("cycle",))
    for n in PLACE_NOPS:
        c[f"place[{n}]"] = Case(place_case(n), dict(path="pt"), ())
    return c


def raw_rows(h):
    """Every valid row a raw build emits (src << 32 | dst, duplicates kept): a
    vectorised count for the histories too large for the Python model."""
    key, txn = np.asarray(h.key, np.uint64), np.asarray(h.txn, np.uint64)
    obs, w = np.asarray(h.observed, np.int64), np.asarray(h.is_write) != 0
    _, kidx = np.unique(key, return_inverse=True)
    kidx = kidx.astype(np.uint64) << np.uint64(32)
    W = np.unique(kidx[w] | txn[w])
    same = (W[:-1] >> np.uint64(32)) == (W[1:] >> np.uint64(32))
    lo32 = np.uint64(0xFFFFFFFF)
    out = [((W[:-1] & lo32) << np.uint64(32) | (W[1:] & lo32))[same]]
    r, rk, ro = txn[~w], kidx[~w], obs[~w]
    wr = (ro >= 0) & (ro != r.astype(np.int64))
    out.append((ro[wr].astype(np.uint64) << np.uint64(32)) | r[wr])
    probe = rk | np.where(ro >= 0, ro, 0).astype(np.uint64)
    pos = np.where(ro >= 0, np.searchsorted(W, probe, side="right"), np.searchsorted(W, probe, side="left"))
    ok = pos < len(W)
    nxt = W[np.minimum(pos, max(len(W) - 1, 0))] if len(W) else np.zeros(len(pos), np.uint64)
    ok &= ((nxt >> np.uint64(32)) == (rk >> np.uint64(32))) & ((nxt & lo32) != r)
    out.append((r[ok] << np.uint64(32)) | (nxt[ok] & lo32))
    return np.concatenate(out)


def valid_raw_rows(h):
    return len(raw_rows(h))


def big_cut_history():
    """any_observed[12] scaled until its valid raw rows pass the fast cut's 65536."""
    return any_observed(12, nops=56000, seed=8)


def ring_history(n_rings=50, base=8192):
    """n_rings disjoint 3-txn rings a < b < c, each held by one ww row (a -> b:
    both write K1, a twice), one wr row (b -> c: c reads b's K2) and one rw row
    (c -> a: c reads the initial K3, which a overwrites) -- the only backward
    edge, covering [a, c] -- with two txns of an acyclic chain (one key, each
    reading its predecessor's write) inside every ring's interval, so their
    rows enter the cut too.  Every writer's txn carries bit 13 and every key
    bit 60; the ops are in txn order."""
    rows, rings = [], []
    kbit = 1 << 60
    prev = -1
    for i in range(n_rings):
        a, b, c = base + 5 * i, base + 5 * i + 2, base + 5 * i + 4
        k1, k2, k3 = (kbit | (8 * i + j) << 3 for j in (1, 2, 3))
        rows += [(a, k1, "w", -1), (a, k3, "w", -1), (a, k1, "w", -1)]
        rows += [(b, k1, "w", -1), (b, k2, "w", -1)]
        rows += [(c, k2, "r", b), (c, k3, "r", -1)]
        for ch in (a + 1, a + 3):
            rows += [(ch, kbit | 7, "r", prev), (ch, kbit | 7, "w", -1)]
            prev = ch
        rings.append((a, b, c))
    rows.sort(key=lambda r: r[0])
    return hist(rows, base + 5 * n_rings + 40), rings


def scc_limit_case(n_nodes, m=None, ntxn=6000, seed=5):
    """A synthetic cut for scc_cut's one-workgroup limits (4096 nodes, 24576
    rows): n_nodes covered txns scattered over ntxn, joined into many 3- and
    4-rings (some linked one way to the next ring) and acyclic chains; the rows
    padded with ~0 and duplicates to m (default: 7 pads).  Returns (cover u8,
    rows i64, (src, dst) distinct edges sorted for the oracle)."""
    rng = np.random.default_rng(seed)
    nodes = rng.permutation(np.sort(rng.choice(ntxn, size=n_nodes, replace=False))).tolist()
    E, i, ring, heads = [], 0, 0, []
    while i + 4 <= (3 * n_nodes) // 4:
        k = 3 + ring % 2
        g = nodes[i:i + k]
        E += [(g[j], g[(j + 1) % k]) for j in range(k)]
        if ring % 5 and heads:
            E.append((heads[-1], g[1]))  # into the next ring, never back
        heads.append(g[0])
        i, ring = i + k, ring + 1
    while i < n_nodes:
        g = nodes[i:i + 5]
        E += list(zip(g, g[1:]))
        i += 5
    E = sorted(set(E))
    s = np.array([a for a, _ in E], np.uint32)
    d = np.array([b for _, b in E], np.uint32)
    base = (s.astype(np.int64) << 32) | d.astype(np.int64)
    m = len(base) + 7 if m is None else m
    assert m >= len(base)
    pad = m - len(base)
    extra = np.concatenate([np.full(pad - pad // 2, -1, np.int64), base[rng.integers(0, len(base), size=pad // 2)]])
    rows = rng.permutation(np.concatenate([base, extra]))
    cover = np.zeros(ntxn, np.uint8)
    cover[nodes] = 1
    return cover, rows, (s, d)
