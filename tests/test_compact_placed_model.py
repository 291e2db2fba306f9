"""CPU: the integer model and the generator of the placed compact-bound tests
(tests/compact_placed.py) -- the model against the CPU sort-join
(oracle/sortjoin.c) for every case and batch order, every placed bound against
the rule restatement of tests/test_compact_model.py, the branch tags the
generator attaches against the tags computed from (X, C, M), their coverage
per width case, the verdict balance, and the point-index placements."""

import numpy as np
import pytest

import compact_placed as P
from test_compact_model import bound

# tags a width case cannot hold: a step that carries or borrows across a code
# word needs a prefix of more than 64 varying bits
SHORT = {f"pre:{c}/x{x}" for c in ("carry", "borrow") for x in (0, 1)}
IMPOSSIBLE = {"w2-63": SHORT, "w3-64": SHORT, "w3-62": SHORT}


def sortjoin(oracle_mod, rows, ngroups, batches):
    sj = oracle_mod.SortJoin(rows.gid, rows.words, rows.lsn, ngroups)
    try:
        return [sj.probe(m, np.zeros(8, np.uint64), nthreads=4)[0] != 0 for m in batches]
    finally:
        sj.close()


@pytest.mark.parametrize("name", P.NAMES)
def test_model_equals_the_sortjoin(oracle_mod, name):
    """Inclusive bounds, strict lsn > snap, one range per read set: the model's
    verdicts are the sort-join's in every order, and 20 .. 80 % conflict."""
    c = P.case(name)
    model = c.model()
    batches = [c.batch(o) for o in P.ORDERS]
    for o, m, want in zip(P.ORDERS, batches, sortjoin(oracle_mod, c.rows, len(c.groups), batches)):
        assert m["n"] == m["n_txn"] and (m["txn"] == np.arange(m["n"])).all()
        np.testing.assert_array_equal(model.verdicts(m), want, err_msg=o)
        assert 0.2 <= want.mean() <= 0.8, (o, want.mean())
    base = c.batch("shuffle")
    assert 300 <= base["n"] <= 6000
    # a batch order only moves read sets
    idx = c.order("shuffle")
    v = model.verdicts(base)
    first = c.batch("points-first")
    pos = {i: t for t, i in enumerate(idx)}
    np.testing.assert_array_equal(model.verdicts(first), v[[pos[i] for i in c.order("points-first")]])


@pytest.mark.parametrize("name", P.NAMES)
def test_windows_are_as_the_cases_say(name):
    c = P.case(name)
    cw, tkw = P.EXPECT[name]
    assert (c.code_words if c.compact else None) == cw and c.tile_key_words == tkw
    assert c.n <= 4100 and len(c.groups) >= (1 if c.alone else 2)
    for gi, g in enumerate(c.g):
        if g is None:
            continue
        assert len(g.rows) == 1 if g.bits == 0 else 40 <= len(g.rows) <= 300
        assert all(r >> g.low << g.low == r for r in g.rows)      # zero past the key length
        acc = 0
        for r in g.rows:
            acc |= r ^ g.rows[0]
        assert acc == g.M and bin(g.M).count("1") == g.bits
    if not c.alone:
        assert c.g[c.norows] is None and c.g[c.single].bits == 0
        assert c.g[c.lowbits].bits + 50 < c.maxbits or name == "w3-62"
    lsn = c.rows.lsn
    assert len(np.unique(lsn)) == c.n
    order = np.argsort(lsn)
    assert not (np.diff(order) == 1).all()                         # scrambled against key order
    for o in P.ORDERS:                                             # zero words past the key length
        m = c.batch(o)
        wl = np.array([(k + 7) // 8 for _, _, k in c.groups])[m["gid"]]
        for j in range(c.W):
            assert not m["lo"][j][wl <= j].any() and not m["hi"][j][wl <= j].any()


def test_window_sizes():
    ns = {name: P.case(name).n for name in P.NAMES}
    assert sum(n >= 2049 for n in ns.values()) >= 1, ns            # two compact tiles
    many = P.case("w8-many")
    assert len(many.groups) >= 90 and many.W == 8


@pytest.mark.parametrize("name", P.NAMES)
def test_bounds_take_their_branches(name):
    """Every placed bound: the rule's lo' / hi' count the rows as the integers
    do, the tag the generator attached is one the bound has, and every tag the
    width allows occurs in a lo and in a hi bound."""
    c = P.case(name)
    roles = {}
    for bi, role in c.meta:
        if bi is not None:
            roles.setdefault(bi, set()).add(role)
    seen = set()
    codes = {gi: [P.gather(r, c.g[gi].V) for r in c.g[gi].rows] for gi in c.placed_groups}
    for bi, (gi, X, tag) in enumerate(c.bounds):
        g = c.g[gi]
        assert tag in P.classify(X, g), (tag, P.classify(X, g))
        assert X & ~g.valid == 0
        lt, le = sum(r < X for r in g.rows), sum(r <= X for r in g.rows)
        lo, hi = bound(X, g.C, g.M, g.nb, g.V, 1), bound(X, g.C, g.M, g.nb, g.V, 2)
        assert lt == (len(g.rows) if lo is None else sum(x < lo for x in codes[gi]))
        assert le == (0 if hi is None else sum(x <= hi for x in codes[gi]))
        assert roles[bi] >= {"lo", "hi"}
        seen.add(tag)
    want = set(P.TAGS) - IMPOSSIBLE.get(name, set())
    assert want <= seen, sorted(want - seen)
    assert not seen & IMPOSSIBLE.get(name, set())


@pytest.mark.parametrize("name", [n for n in P.NAMES if 1 <= P.EXPECT[n][1] <= 3 and P.SPECS[n]["W"] <= 8
                                  and not P.SPECS[n].get("alone")])
def test_point_index_placements(name):
    """Under the restated hash nine rows share one home bucket (two full lines
    are walked) and five are homed in the last bucket (the walk wraps)."""
    c = P.case(name)
    g = c.g[c.pg]
    home = lambda r: P.point_home(c.pg, P.gather(r, g.V), g.bits, c.code_words, c.gb, c.tile_key_words, c.n)
    same = {home(r) for r in c.point_rows["same"]}
    assert len(c.point_rows["same"]) == 9 and len(same) == 1 and same != {c.n + 63}
    assert len(c.point_rows["last"]) == 5 and {home(r) for r in c.point_rows["last"]} == {c.n + 63}
    assert set(c.point_rows["same"] + c.point_rows["last"]) <= g.rowset
    absent = c.point_rows["absent"]
    assert len(absent) == 3 and not set(absent) & g.rowset
    assert {home(r) for r in absent} == same | {c.n + 63}
    assert all((r ^ g.C) & ~g.M == 0 for r in absent)             # on the pattern
    assert sum(home(r) in same for r in g.rows) >= 9


def test_rebuild_case(oracle_mod):
    c = P.rebuild_case()
    k = [set(P.from_words(c.rows(w).words)) for w in (0, 1)]
    assert len(c.rows(0)) == len(c.rows(1)) and not k[0] & k[1]
    for w in (0, 1):
        m = c.batch(w)
        want, = sortjoin(oracle_mod, c.rows(w), len(c.GROUPS), [m])
        np.testing.assert_array_equal(P.Model(c.W, c.rows(w)).verdicts(m), want)
        assert 0.2 <= want.mean() <= 0.8
        assert (m["lo"] == m["hi"]).all()
