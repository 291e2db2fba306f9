"""GPU: placed probes of the rows appended after a window build -- the delta
runs (hsc_delta.hip k_delta_merge / k_probe_delta, delta_hit in hsc_device.h),
the second half of the small-batch kernel (hsc_narrow.hip delta_range16,
pend_range16, small_appended16 and its WD == 0 branch), the pack after the
delta probe on every layout, folds and the rw pairs after appends -- bit for
bit against the numpy model of tests/appended_model.py (pinned to the CPU
sort-join by tests/test_appended_model.py).

Every case runs on a context of its own.  The main window is small (int64 keys
with stride 7, ingested as device rows), appended keys fall between its keys
and onto some.  A read set is one range or one table lock; its snapshot is the
LSN of the newest row its range holds (no conflict) or the LSN before it (a
conflict), and never older than a main-window row except where a case says so:
a kernel that is off by one row, counts a straddling 64-row block in, takes
the block maximum over other rows, lets a neighbouring group's equal key words
match or drops the row equal to a bound fails here."""

import ctypes

import numpy as np
import pytest

import appended_model as A
from comdb2_amd.formats import KEY_NULL, ReadSets
from comdb2_amd.hsc import (LAYOUT_AUTO, LAYOUT_COMPACT, LAYOUT_NARROW, LAYOUT_NARROW_TILES, LAYOUT_WIDE,
                            PATH_NO_SMALL, Validator)
from test_gpu_ingest import _reference
from test_gpu_join_column import launch, outputs, result, upload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

INT64_GROUP = [("t1", 0, A.INT64_KLEN)]
SMALL_MAX = 1024        # read sets of one small-batch call
RUN_CAP = 65536         # hsc_set_fold's largest row count


# ---- contexts ----------------------------------------------------------------
@pytest.fixture
def ctx():
    """ctx(groups, layout, paths, fold) -> a Validator of its own, closed after the test."""
    made = []

    def make(groups=INT64_GROUP, layout=LAYOUT_AUTO, paths=0, fold=(RUN_CAP, False)):
        v = Validator(0)
        made.append(v)
        for g, (tb, ix, klen) in enumerate(groups):
            assert v.register_group(tb, ix, klen) == g
        v.set_layout(layout)
        v.set_paths(paths)
        v.set_fold(*fold)
        return v

    yield make
    for v in made:
        v.close()


def ingest(v, rows, layout=LAYOUT_NARROW):
    """The main window as device rows (hsc_window_ingest_device); `layout`: what it must come out as."""
    dev = torch.device("cuda", 0)
    tg = torch.from_numpy(rows.gid.astype(np.int32)).to(dev)
    tw = torch.from_numpy(rows.words.reshape(-1).view(np.int64)).to(dev)
    tl = torch.from_numpy(rows.lsn.view(np.int64)).to(dev)
    v.ingest_device(len(rows), rows.words.shape[0], tg.data_ptr(), tw.data_ptr(), tl.data_ptr(), A.END)
    torch.cuda.synchronize()
    assert v.words == rows.words.shape[0] and v.layout == layout


_WRITE = np.dtype({"names": ["tbname", "idxnum", "key", "keylen", "lsn"],
                   "formats": [np.uint64, np.int32, np.uint64, np.int32, np.uint64],
                   "offsets": [0, 8, 16, 24, 32], "itemsize": 40})  # hsc_write


def append(v, rows, groups=INT64_GROUP):
    """One hsc_window_append of `rows` in their order."""
    n = len(rows)
    klen = groups[0][2]
    assert all(g[2] == klen for g in groups)
    kb = A.words_bytes(rows.words, klen)
    names = [ctypes.create_string_buffer(tb.encode()) for tb, _, _ in groups]
    w = np.zeros(n, _WRITE)
    w["tbname"] = np.array([ctypes.addressof(x) for x in names], np.uint64)[rows.gid]
    w["idxnum"] = np.array([g[1] for g in groups], np.int32)[rows.gid]
    w["key"] = kb.ctypes.data + klen * np.arange(n, dtype=np.uint64)
    w["keylen"] = klen
    w["lsn"] = rows.lsn
    v._chk(v.lib.hsc_window_append(v.ctx, w.ctypes.data, n), "hsc_window_append")


def append_to_run(v, rows, groups=INT64_GROUP):
    """Append with the small path off: the rows go to the run, not the pending tail."""
    v.set_paths(PATH_NO_SMALL)
    append(v, rows, groups)
    v.set_paths(0)
    assert v.append_stats()["pending_rows"] == 0


# ---- read sets of a batch of probe columns -----------------------------------
def readsets(m, groups):
    """ReadSets of the batch `m` (read set t = range t, then one lock each;
    table g = group g's), with full-length keys."""
    n, nl = m["n"], m["n_lock"]
    klen = groups[0][2]
    lk, hk = A.words_bytes(m["lo"], klen), A.words_bytes(m["hi"], klen)
    i32 = lambda a, fill=0: np.concatenate([np.asarray(a, np.int32), np.full(nl, fill, np.int32)])
    off = klen * np.arange(n, dtype=np.uint64)
    null = np.full(nl, KEY_NULL, np.uint64)
    return ReadSets(txn_off=np.arange(n + nl + 1, dtype=np.int64),
                    snap=np.concatenate([m["snap"], m["lock_snap"]]),
                    table=np.concatenate([m["gid"].astype(np.int32), m["lock_table"].astype(np.int32)]),
                    idxnum=i32(np.array([g[1] for g in groups], np.int32)[m["gid"]], -2), lflag=i32(np.zeros(n), 1),
                    rflag=i32(np.zeros(n), 1), islocked=i32(np.zeros(n), 1),
                    lkeylen=i32(np.full(n, klen)), rkeylen=i32(np.full(n, klen)),
                    lkey_off=np.concatenate([off, null]), rkey_off=np.concatenate([off + np.uint64(klen * n), null]),
                    keys=np.concatenate([lk.reshape(-1), hk.reshape(-1), np.zeros(1, np.uint8)]),
                    tbnames=[g[0] for g in groups])


def same_columns(got, m):
    """The marshalled read sets are the batch's columns: the model sees what the kernel sees."""
    assert (got["words"], got["n"], got["n_lock"], got["n_txn"]) == (m["words"], m["n"], m["n_lock"], m["n_txn"])
    o = np.argsort(got["txn"], kind="stable")
    np.testing.assert_array_equal(got["txn"][o], m["txn"])
    for k in ("gid", "snap"):
        np.testing.assert_array_equal(got[k][o], m[k])
    for k in ("lo", "hi"):
        np.testing.assert_array_equal(got[k][:, o], m[k])
    o = np.argsort(got["lock_txn"], kind="stable")
    for k in ("lock_txn", "lock_table", "lock_snap"):
        np.testing.assert_array_equal(got[k][o], m[k])
    assert not got["forced"].any()


def check_small(v, m, groups=INT64_GROUP):
    """Verdicts of `m` through hsc_check_readsets in calls of <= 1024 read sets,
    every call on the small path."""
    parts = [m] if m["n_txn"] <= SMALL_MAX else [A.slice_batch(m, a, min(a + SMALL_MAX, m["n"]))
                                                 for a in range(0, m["n"], SMALL_MAX)]
    calls = v.small_stats()["calls"]
    out = []
    for p in parts:
        rs = readsets(p, groups)
        same_columns(v.marshal(rs), p)
        out.append(v.check_readsets(rs) != 0)
    assert v.small_stats()["calls"] == calls + len(parts), "a call left the small path"
    return np.concatenate(out)


def check_staged(v, m, groups=INT64_GROUP):
    """The same through the staged path (k_probe_delta); no call is small."""
    calls = v.small_stats()["calls"]
    rs = readsets(m, groups)
    same_columns(v.marshal(rs), m)
    got = v.check_readsets(rs) != 0
    assert v.small_stats()["calls"] == calls
    return got


def probe(v, m):
    """hsc_probe_device into verdict bytes of 0xFF and a bitmap of ones."""
    u, out = upload(m), outputs(m)
    torch.cuda.synchronize()
    launch(v, m, u, out)
    torch.cuda.synchronize()
    return result(m, *out)


def expect(got, model, m, table_max=None):
    want = model.verdicts(m, table_max)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} of {len(want)} read sets differ, first {bad[:8].tolist()}: " \
                          f"want {want[bad[:8]].tolist()}"


# ---- (a) search positions on the small path --------------------------------------
@pytest.mark.parametrize("n", A.SEARCH_SIZES)
def test_search_positions(ctx, n):
    """delta_range16's 16-ary searches: every row of a run of n rows alone, at
    its LSN and the LSN before, and the gap after it."""
    c = A.SearchCase(n)
    v = ctx()
    ingest(v, c.main)
    append_to_run(v, c.appends)
    assert v.delta_rows == n
    m = c.probes(np.arange(n))
    expect(check_small(v, m), c.model(), m)
    assert v.delta_rows == n and v.fold_stats()["inline"] == 0


def test_search_positions_largest_run(ctx):
    """The largest run a probe sees with set_fold(65536, inline): one row below
    the fold's row count (a run of that many rows is folded by the next check)."""
    c = A.SearchCase(RUN_CAP - 1)
    v = ctx()
    ingest(v, c.main)
    append_to_run(v, c.appends)
    n = v.delta_rows
    assert n == c.n
    rows = c.boundary_rows()
    m = c.probes(rows)
    model = c.model()
    expect(check_small(v, m), model, m)
    assert v.delta_rows == n and v.fold_stats()["inline"] == 0  # every probe met the whole run
    # one more row: the next check folds the run
    top = A.Rows(np.zeros(1, np.uint32), A.int64_words(c.keys[-1:] + A.APP_STEP), [A.END + n])
    append_to_run(v, top)
    model.append(top)
    assert v.delta_rows == n + 1
    m = c.probes(rows[:300])
    expect(check_small(v, m), model, m)
    assert v.delta_rows == 0 and v.fold_stats()["inline"] == 1


# ---- (b) head / whole blocks / tail ------------------------------------------------
@pytest.fixture(scope="module")
def block_case():
    c = A.BlockCase()
    return c, c.model(), c.probes()


@pytest.mark.parametrize("consumer", ["small", "device", "staged"])
def test_head_blocks_tail(ctx, block_case, consumer):
    """Ranges [pa, pb) with pa % 64, pb % 64 in {0, 1, 63} over 0, 1, 2 and 5
    whole blocks, the newest row at each end of the head, the blocks and the
    tail, the rows pa - 1 and pb newer than every snapshot: delta_range16
    (small), delta_hit in k_probe_delta (device probe, staged check)."""
    c, model, m = block_case
    v = ctx(paths=0 if consumer == "small" else PATH_NO_SMALL)
    ingest(v, c.main)
    append(v, c.appends)
    assert v.delta_rows == c.n >= 1024 and v.append_stats()["pending_rows"] == 0
    got = {"small": check_small, "device": probe, "staged": check_staged}[consumer](v, m)
    expect(got, model, m)
    assert v.delta_rows == c.n


# ---- (c) groups and key words ---------------------------------------------------------
@pytest.mark.parametrize("vary", A.VARY)
@pytest.mark.parametrize("W", A.WIDTHS)
def test_groups_and_words(ctx, W, vary):
    """Three groups with the same key words: only group 1's rows answer group
    1's ranges.  W <= 4 runs small_appended16<W>, W = 5 and 9 the WD == 0
    branch (delta_hit inside the small kernel, no pending tail); W = 9 merges
    from uploaded rows (past the in-place staging's W <= 8)."""
    c = A.GroupCase(W, vary)
    groups = [(tb, 0, c.klen) for tb in ("ta", "tb", "tc")]
    v = ctx(groups)
    ingest(v, c.main)
    before = v.append_stats()
    append(v, c.appends, groups)  # more rows than the tail takes: merged at once
    st = v.append_stats()
    assert st["pending_rows"] == 0 and st["pending_appends"] == before["pending_appends"]
    assert v.delta_rows == 3 * c.n and v.words == W
    model, m = c.model(), c.probes()
    expect(check_small(v, m, groups), model, m)
    expect(probe(v, m), model, m)
    if W > 4:  # no tail for these widths: a commit's few rows are merged by the append
        few = A.Rows(np.ones(2, np.uint32), A.vary_words(W, vary, [5, 11]), [A.END + 3 * c.n, A.END + 3 * c.n + 1])
        append(v, few, groups)
        model.append(few)
        st = v.append_stats()
        assert st["pending_rows"] == 0 and st["pending_appends"] == before["pending_appends"]
        assert v.delta_rows == 3 * c.n + 2
        new = A.batch(W, np.array([1, 1, 0, 2], np.uint32), A.vary_words(W, vary, [5, 5, 5, 11]),
                      A.vary_words(W, vary, [11, 11, 11, 11]),
                      [A.END + 3 * c.n + 1, A.END + 3 * c.n, A.END + 3 * c.n - 1, A.END + 3 * c.n - 1])
        np.testing.assert_array_equal(model.verdicts(new), [False, True, False, False])
        expect(check_small(v, new, groups), model, new)


# ---- (d) the pending tail -----------------------------------------------------------
@pytest.mark.parametrize("n", A.PENDING_SIZES)
def test_pending_tail(ctx, n):
    """n rows appended a few at a time stay in the pending tail (pend_range16
    scans them from LDS, table locks read the pending table maxima), then merge
    into the run with the same verdicts."""
    c = A.PendingCase(n)
    v = ctx()
    ingest(v, c.main)
    at = 0
    for k in c.pieces():
        append(v, c.appends.take(np.arange(at, at + k)))
        at += k
        assert v.append_stats()["pending_rows"] == at
    st = v.append_stats()
    assert st["pending_appends"] == len(c.pieces()) and st["pending_merges"] == 0 and v.delta_rows == n
    model = c.model()
    tm = model.table_max([0], 1)
    batches = (c.probes(np.arange(n)), c.bound_probes(), c.lock_probes())
    for m in batches:
        expect(check_small(v, m), model, m, tm)
    assert v.append_stats() == st  # still waiting: every check scanned the tail
    # one more row; a batch that is not small (or a full tail) merges the tail into the run
    top = A.Rows(np.zeros(1, np.uint32), A.int64_words(c.keys[-1:] + 10 * A.APP_STEP), [A.END + n])
    append(v, top)
    model.append(top)
    probe(v, batches[0])
    st2 = v.append_stats()
    assert st2["pending_rows"] == 0 and st2["pending_merges"] > st["pending_merges"] and v.delta_rows == n + 1
    tm = model.table_max([0], 1)
    for m in batches:
        expect(check_small(v, m), model, m, tm)


# ---- (e) merge variants --------------------------------------------------------------
@pytest.mark.parametrize("steps", [A.MERGE_STEPS, (40500, 256)], ids=["sizes", "long-run"])
def test_merge_variants(ctx, steps):
    """k_delta_merge without a tail: appends of 1, 255 and 256 rows staged in
    LDS from mapped host memory, 257 and 3000 rows uploaded, onto runs of 0, 63,
    64, 65 and 256 rows; 256 rows onto a run past the in-place byte rule
    (uploaded); keys that come again and main-window keys.  After every append
    the block-boundary ranges of the run so far."""
    c = A.StreamCase(steps)
    v = ctx(paths=PATH_NO_SMALL)
    ingest(v, c.main)
    model = A.Model(2, c.main)
    for p in c.pieces():
        append(v, p)
        model.append(p)
        assert v.delta_rows == len(model.app) and v.append_stats()["pending_appends"] == 0
        m, _, _ = A.boundary_probes(model.run(), 2)
        expect(probe(v, m), model, m)
    assert v.fold_stats()["inline"] == 0


# ---- (g) folds -------------------------------------------------------------------------
def expect_export(v, model):
    u = model.main.cat(model.app)
    want_all, want_new = _reference(u.gid, u.words, u.lsn)
    for got, want in ((v.export_window(True), want_all), (v.export_window(False), want_new)):
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)


def test_inline_folds(ctx):
    """Three inline folds of a 600-row run (the check after the append that
    fills it folds; hsc_probe_device takes built windows only): the folded
    window is the sort of the union, every version and the newest per key."""
    c = A.StreamCase(A.FOLD_STEPS)
    v = ctx(paths=PATH_NO_SMALL, fold=(600, False))
    ingest(v, c.main)
    model = A.Model(2, c.main)
    folds = 0
    for p in c.pieces():
        append(v, p)
        model.append(p)
        m, _, _ = A.boundary_probes(model.run(), 2)
        expect(check_staged(v, m), model, m)
        if v.fold_stats()["inline"] > folds:
            folds += 1
            assert v.delta_rows == 0
            expect_export(v, model)
    assert folds == 3


def test_background_folds(ctx):
    """The same appends with background folds: verdicts equal the model whether
    a check met the frozen run or the swapped window."""
    c = A.StreamCase(A.FOLD_STEPS)
    v = ctx(paths=PATH_NO_SMALL, fold=(600, True))
    ingest(v, c.main)
    model = A.Model(2, c.main)
    frozen = 0
    for p in c.pieces():
        append(v, p)
        model.append(p)
        m, _, _ = A.boundary_probes(model.run(), 2)
        st = v.fold_stats()
        frozen += st["started"] > st["swapped"]
        expect(probe(v, m), model, m)
    print(f"checks that met a frozen run: {frozen} of {len(c.steps)}")
    expect_export(v, model)
    assert v.delta_rows == 0
    assert v.fold_stats()["started"] >= 1


# ---- (f) the device probe with a run: verdict bytes, bitmap, cleared read sets ------------
def device_case(path):
    return A.compact_device_case() if path == "compact" else A.int64_device_case()


@pytest.mark.parametrize("path", ["column", "plan", "wide", "compact"])
def test_device_probe_with_a_run(ctx, path):
    """hsc_probe_device with a run beside the window, into verdict bytes of
    0xFF and a bitmap of ones (the pack runs after the delta probe): read sets
    conflicting in the main window only, in the run only, in both, in neither,
    without a range, and table locks, for 1, 63, 64, 65 and 4097 read sets.
    Narrow tiles: the join that scans its own column and the plan path (after
    a batch with a tile past 1024 records); the wide layout; a window of
    compact tiles (its batches of up to 65 read sets are sparse: they take the
    wide pipeline over compact codes, 4097 read sets the compact tiles)."""
    c = device_case(path)
    groups = [("t1", 0, 23)] if path == "compact" else INT64_GROUP
    layout = {"column": LAYOUT_NARROW_TILES, "plan": LAYOUT_NARROW_TILES, "wide": LAYOUT_WIDE,
              "compact": LAYOUT_AUTO}[path]
    v = ctx(groups, layout=layout)
    ingest(v, c.main, {"wide": LAYOUT_WIDE, "compact": LAYOUT_COMPACT}.get(path, LAYOUT_NARROW))
    append(v, c.appends, groups)
    assert v.delta_rows == c.n and v.append_stats()["pending_rows"] == 0
    model = c.model()
    tm = model.table_max([0], 1)
    if path == "compact":
        assert 1 <= v.tile_key_words <= 3
    stats = lambda: (v.batch_stats()["column_batches"], v.batch_stats()["plan_batches"])
    if path == "plan":  # 1200 records in the first tile: the batches after it take the plan
        r = 1 + (3 * np.arange(1200)) % 3000
        keys = A.main_keys(len(c.main))
        lo, hi = A.int64_words(keys[r] - 1), A.int64_words(keys[r + 2] + 1)
        snap = model.range_max(np.zeros(1200, np.uint32), lo, hi) - (np.arange(1200) % 2).astype(np.uint64)
        hot = A.batch(2, np.zeros(1200, np.uint32), lo, hi, snap)
        expect(probe(v, hot), model, hot)
        assert stats() == (1, 0)
    done = stats()
    for T in A.DEVICE_TXNS:
        m, kind = c.batch(T)
        got = probe(v, m)
        expect(got, model, m, tm)
        assert got[kind <= 2].all() and not got[(kind == 3) | (kind == 4)].any()
        if path in ("column", "plan"):
            done = (done[0] + (path == "column"), done[1] + (path == "plan"))
            assert stats() == done
    assert v.delta_rows == c.n
