"""CPU: the appended-row model (tests/appended_model.py) against the CPU
sort-join (oracle/sortjoin.c) built over the same union of main-window and
appended rows, for every generator of the placed GPU tests
(tests/test_gpu_appended_placed.py), and the generators' own conditions: the
(pa % 64, pb % 64, whole blocks) classes are produced, 40 .. 60 % of the placed
read sets conflict, and no snapshot is older than a main-window row, so every
verdict is the appended rows' alone."""

import numpy as np
import pytest

import appended_model as A
from comdb2_amd.workloads import int64_words


def sortjoin_verdicts(oracle_mod, model, m, table_max=(), ngroups=1):
    u = model.main.cat(model.app)
    sj = oracle_mod.SortJoin(u.gid, u.words, u.lsn, ngroups)
    try:
        want, _ = sj.probe(m, np.asarray(table_max, np.uint64), nthreads=4)
    finally:
        sj.close()
    return want != 0


def check_placed(oracle_mod, model, m, table_max=(), ngroups=1, holds_rows=None):
    """The model equals the sort-join; no read set conflicts through the main
    window; 40 .. 60 % of the read sets whose range holds an appended row (all
    without `holds_rows`) conflict.  -> the verdicts."""
    got = model.verdicts(m, table_max)
    np.testing.assert_array_equal(got, sortjoin_verdicts(oracle_mod, model, m, table_max, ngroups))
    main_top = int(model.main.lsn.max())
    assert main_top < A.END
    assert int(m["snap"].min(initial=A.END)) >= main_top
    assert int(m["lock_snap"].min(initial=A.END)) >= main_top
    main_only = A.Model(model.W, model.main)
    assert not main_only.verdicts(m, np.zeros(max(1, len(table_max)), np.uint64)).any()
    placed = got if holds_rows is None else got[holds_rows]
    assert 0.4 <= placed.mean() <= 0.6, placed.mean()
    if holds_rows is not None:
        assert not got[~holds_rows].any()
    return got


def test_keys_order_as_composites():
    assert (A.int64_words(np.array([-5, 0, 1, 1000, 2 ** 40, -2 ** 62])) ==
            int64_words(np.array([-5, 0, 1, 1000, 2 ** 40, -2 ** 62]))).all()
    rng = np.random.default_rng(1)
    gid = rng.integers(0, 3, 400).astype(np.uint32)
    # bytes 0x00, 0x7F, 0x80 and 0xFF in every place: signed or NUL-ended compares would differ
    words = rng.choice(np.array([0, 0x7F, 0x80, 0xFF, 0x8000000000000000, 0xFF00000000000000,
                                 0x00FF000000000000], np.uint64), (3, 400))
    k = A.row_keys(gid, words)
    tup = [(int(gid[i]),) + tuple(int(x) for x in words[:, i]) for i in range(400)]
    order = np.argsort(k, kind="stable")
    assert [tup[i] for i in order] == sorted(tup)
    assert order.tolist() == sorted(range(400), key=lambda i: (tup[i], i))
    for i in range(0, 400, 7):
        assert int(np.searchsorted(k[order], k[i], "left")) == sum(t < tup[i] for t in tup)
        assert int(np.searchsorted(k[order], k[i], "right")) == sum(t <= tup[i] for t in tup)


def test_model_equals_the_definition(oracle_mod):
    """Small batches, row by row: ranges, repeated keys, table locks, forced verdicts."""
    c = A.StreamCase((5, 40, 7), nmain=60)
    model = A.Model(2, c.main)
    for p in c.pieces():
        model.append(p)
    m, _, _ = A.boundary_probes(model.run(), 2)
    tm = model.table_max([0], 1)
    assert int(tm[0]) == A.END + 51
    lk = A.batch(2, m["gid"], m["lo"], m["hi"], m["snap"], [0, 0], [int(tm[0]), int(tm[0]) - 1])
    lk["forced"][3] = 1
    want = model.verdicts_brute(lk, tm)
    np.testing.assert_array_equal(model.verdicts(lk, tm), want)
    np.testing.assert_array_equal(sortjoin_verdicts(oracle_mod, model, lk, tm), want)
    assert want[3] and want[-1] and not want[-2]


@pytest.mark.parametrize("n", A.SEARCH_SIZES + (65535,))
def test_search_positions(oracle_mod, n):
    c = A.SearchCase(n)
    model = c.model()
    run = model.run()
    assert (run.lsn == c.lsn).all() and (run.words == A.int64_words(c.keys)).all()
    rows = np.arange(n) if n <= 4097 else c.boundary_rows()
    if n > 4097:
        for mod in (16, 256, 4096):
            for d in (-2, -1, 0, 1, 2):
                want = np.arange(mod, n, mod) + d
                assert np.isin(want[want < n], rows).all()
        assert len(rows) >= 5 * (n // 16) + 2048
    m = c.probes(rows)
    pa, pb = model.positions(run, m["gid"], m["lo"], m["hi"])
    np.testing.assert_array_equal(pa[0::3], rows)        # the row alone ...
    np.testing.assert_array_equal(pb[0::3], rows + 1)
    np.testing.assert_array_equal(pa[2::3], rows + 1)    # ... and the gap after it
    np.testing.assert_array_equal(pb[2::3], rows + 1)
    holds = pb > pa
    got = check_placed(oracle_mod, model, m, holds_rows=holds)
    assert got[1::3].all() and not got[0::3].any()
    # some appended keys are main-window keys, most are not
    on_main = np.isin(c.keys, A.main_keys(len(c.main)))
    assert n < 16 or 0 < on_main.sum() < n


def test_head_blocks_tail(oracle_mod):
    c = A.BlockCase()
    assert 1024 <= c.n < 65536
    model = c.model()
    run = model.run()
    assert (run.lsn == c.lsn).all()
    m = c.probes()
    pa, pb = model.positions(run, m["gid"], m["lo"], m["hi"])
    seen = set()
    for q, (a, b, B, where, ra, rb, newest) in enumerate(c.regions):
        assert (pa[2 * q], pb[2 * q]) == (ra, rb) == (pa[2 * q + 1], pb[2 * q + 1])
        assert (ra % 64, rb % 64, int(A.whole_blocks(np.array([ra]), np.array([rb]))[0])) == (a, b, B)
        assert ra + int(np.argmax(c.lsn[ra:rb])) == newest
        assert int(m["snap"][2 * q]) == int(c.lsn[newest])
        # the rows next to the range are newer than every snapshot in use
        assert min(int(c.lsn[ra - 1]), int(c.lsn[rb])) > int(m["snap"].max())
        seen.add((a, b, B, where))
    for B in A.WHOLE:
        for a in A.OFFSETS:
            for b in A.OFFSETS:
                if B == 0 and a == 0 and b == 0:
                    continue  # no row
                want = {"first", "last"} | ({"last-head"} if a else set()) | \
                       ({"block-first", "block-last"} if B else set()) | ({"first-tail"} if b else set())
                assert {w for (x, y, z, w) in seen if (x, y, z) == (a, b, B)} == want
    got = check_placed(oracle_mod, model, m)
    assert got[1::2].all() and not got[0::2].any()


@pytest.mark.parametrize("vary", A.VARY)
@pytest.mark.parametrize("W", A.WIDTHS)
def test_groups_and_words(oracle_mod, W, vary):
    c = A.GroupCase(W, vary)
    model = c.model()
    m = c.probes()
    assert (m["gid"] == 1).all()
    assert not A.words_bytes(m["lo"], c.klen)[:, c.klen:].any()
    # the same words in every group, with different LSNs
    run = model.run()
    n = c.n
    for g in (1, 2):
        assert (run.words[:, g * n:(g + 1) * n] == run.words[:, :n]).all()
        assert (run.lsn[g * n:(g + 1) * n] != run.lsn[:n]).all()
    got = check_placed(oracle_mod, model, m, ngroups=3)
    pa, pb = model.positions(run, m["gid"], m["lo"], m["hi"])
    assert pa.min() >= n and pb.max() <= 2 * n and int(A.whole_blocks(pa, pb).max()) >= 2
    # a neighbour's row under the same words would change verdicts either way
    for g in (0, 2):
        other = A.batch(W, np.full(m["n"], g, np.uint32), m["lo"], m["hi"], m["snap"])
        diff = model.verdicts(other) != got
        assert diff[got].any() and diff[~got].any()


@pytest.mark.parametrize("n", A.PENDING_SIZES)
def test_pending_tail(oracle_mod, n):
    c = A.PendingCase(n)
    assert sum(c.pieces()) == n and (n < 3 or len(c.pieces()) > 2)
    model = c.model()
    m = c.probes(np.arange(n))
    check_placed(oracle_mod, model, m, holds_rows=np.arange(3 * n) % 3 != 2)
    bp = c.bound_probes()
    got = check_placed(oracle_mod, model, bp, holds_rows=np.arange(6 * n) < 4 * n)
    assert got[n:2 * n].all() and got[3 * n:4 * n].all()
    lk = c.lock_probes()
    tm = model.table_max([0], 1)
    np.testing.assert_array_equal(check_placed(oracle_mod, model, lk, tm), [False, True])
    # the main window alone leaves the table's maximum below both lock snapshots
    assert int(A.Model(2, c.main).table_max([0], 1)[0]) < int(lk["lock_snap"].min())


@pytest.mark.parametrize("steps", [A.MERGE_STEPS, A.FOLD_STEPS, (40500, 256)], ids=["merge", "fold", "long-run"])
def test_append_streams(oracle_mod, steps):
    c = A.StreamCase(steps)
    model = A.Model(2, c.main)
    before, classes = [], set()
    for p in c.pieces():
        before.append(len(model.app))
        model.append(p)
        run = model.run()
        m, pa, pb = A.boundary_probes(run, 2)
        assert (pb > pa).all()
        classes |= set(zip((pa % 64).tolist(), (pb % 64).tolist(), A.whole_blocks(pa, pb).tolist()))
        check_placed(oracle_mod, model, m)
    if steps == A.MERGE_STEPS:
        assert set(before) >= {0, 63, 64, 65, 256} and set(steps) >= {1, 255, 256, 257, 3000}
    if len(model.app) > 1024:
        assert classes >= {(a, b, B) for a in A.OFFSETS for b in A.OFFSETS for B in A.WHOLE} - {(0, 0, 0)}
    keys = c.keys
    assert len(np.unique(keys)) < len(keys)                         # keys written again later ...
    assert np.isin(keys, A.main_keys(len(c.main))).any()            # ... and main-window keys
    # a key's newer version follows the older one in the run
    run = model.run()
    same = (run.words[:, 1:] == run.words[:, :-1]).all(axis=0)
    assert same.any() and (run.lsn[1:][same] > run.lsn[:-1][same]).all()


@pytest.mark.parametrize("make", [A.int64_device_case, A.compact_device_case], ids=["int64", "compact"])
def test_device_probe_kinds(oracle_mod, make):
    """The one generator whose snapshots reach below main-window rows: every
    kind of read set does what its name says."""
    c = make()
    model = c.model()
    tm = model.table_max([0], 1)
    assert int(tm[0]) == A.END + c.n - 1
    run_only = A.Model(c.W)
    run_only.append(c.appends)
    main_only = A.Model(c.W, c.main)
    for T in A.DEVICE_TXNS:
        m, kind = c.batch(T)
        assert m["n"] + m["n_lock"] == int((kind != 4).sum())
        got = model.verdicts(m, tm)
        np.testing.assert_array_equal(got, sortjoin_verdicts(oracle_mod, model, m, tm))
        in_main = main_only.verdicts(m, np.zeros(1, np.uint64))
        in_run = run_only.verdicts(m, run_only.table_max([0], 1))
        lock = kind == 5
        assert in_main[kind == 0].all() and not in_run[kind == 0].any()
        assert in_run[kind == 1].all() and not in_main[kind == 1].any()
        assert in_main[kind == 2].all() and in_run[kind == 2].all()
        assert not got[(kind == 3) | (kind == 4)].any()
        np.testing.assert_array_equal(got[lock], (np.flatnonzero(lock) // 6) % 2 == 1)
        assert not in_main[lock].any()
        if T == 4097:
            assert 0.4 <= got.mean() <= 0.6
