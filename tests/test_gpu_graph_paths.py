"""Every read-search path of the dependency-graph build held to exact oracle
edges (-m gpu).  tests/graph_cases.py builds the histories and predicts the
branch each one reaches (asserted on the CPU by test_graph_cases.py); here
each case is built three ways and compared with oracle/scc_oracle.c:

  full        sorted unique (src, dst, type), the per-type counts, the SCC
  raw_host    the raw rows of an uploaded history: the cover, and the cut
              under an all-ones cover = the oracle's edge set exactly
  raw_device  the same over device-resident ops (the build checks the ops
              itself and finds the txn order: fused ww rows, skipped txn
              bits), and again with a 4-row backward list (interval diffs)

then the cut's flag-and-scan form, buffer reuse across builds, the op-range
cut behind hsc_multi_graph_scc, and the one-workgroup SCC's size limits."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch  # imported before any test initialises HIP

import graph_cases as gc
from comdb2_amd import shard
from test_graph_shard import _cover_of, _multi_scc

pytestmark = pytest.mark.gpu

NAMES = list(gc.cases())
_REF = {}


def _ref(oracle_mod, name, h):
    """The oracle's answer for a history, computed once per name."""
    if name not in _REF:
        s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
        rows = np.unique((s.astype(np.uint64) << np.uint64(32)) | d.astype(np.uint64))
        assert len(rows) == len(s)
        _REF[name] = SimpleNamespace(s=s, d=d, t=t, scc=oracle_mod.scc(h.ntxn, s, d), rows=rows,
                                     cover=_cover_of(zip(s.tolist(), d.tolist()), h.ntxn))
    return _REF[name]


def _check_full(validator, h, r):
    scc, st = validator.dep_graph_scc(h)
    gs, gd, gt = validator.dep_graph_edges()
    np.testing.assert_array_equal(gs, r.s)
    np.testing.assert_array_equal(gd, r.d)
    np.testing.assert_array_equal(gt, r.t)
    np.testing.assert_array_equal(scc, r.scc)
    assert st["edges"] == len(r.s)
    assert [st["ww"], st["wr"], st["rw"]] == [int(((r.t >> k) & 1).sum()) for k in range(3)]


def _cut_rows(g, cover):
    return g.cut(cover).cpu().numpy().view(np.uint64)


def _check_raw(g, built_from, ntxn, r):
    """A raw build's cover and its cut under an all-ones cover."""
    dev = g.device
    g.build(built_from)
    cover = torch.full((max(ntxn, 1),), 7, dtype=torch.uint8, device=dev)
    g.cover(cover)
    np.testing.assert_array_equal(cover[:ntxn].cpu().numpy() != 0, r.cover)
    rows = _cut_rows(g, torch.ones(max(ntxn, 1), dtype=torch.uint8, device=dev))
    assert not (rows == np.uint64(gc.M64)).any()
    np.testing.assert_array_equal(np.unique(rows), r.rows)
    return rows


@pytest.mark.parametrize("name", NAMES)
def test_full_build_matches_oracle(validator, oracle_mod, name):
    h = gc.cases()[name].h
    _check_full(validator, h, _ref(oracle_mod, name, h))


@pytest.mark.parametrize("name", NAMES)
def test_raw_host_build_matches_oracle(validator, oracle_mod, name):
    h = gc.cases()[name].h
    g = shard.GpuGraph(validator, torch.device("cuda", 0))
    _check_raw(g, h, h.ntxn, _ref(oracle_mod, name, h))


@pytest.mark.parametrize("back_cap", [None, 4])
@pytest.mark.parametrize("name", NAMES)
def test_raw_device_build_matches_oracle(validator, oracle_mod, name, back_cap, monkeypatch):
    """back_cap 4: the backward rows past a 4-row list are only counted and
    the cover comes from interval diffs of every raw row -- the same cover."""
    if back_cap is not None:
        monkeypatch.setenv("HSC_GRAPH_BACK_CAP", str(back_cap))
    h = gc.cases()[name].h
    dev = torch.device("cuda", 0)
    g = shard.GpuGraph(validator, dev)
    _check_raw(g, shard.device_history(h, dev), h.ntxn, _ref(oracle_mod, name, h))


@pytest.mark.parametrize("nops", gc.PLACE_NOPS)
def test_raw_device_build_unaligned_is_write(validator, oracle_mod, nops):
    """is_write starting one byte past a 16-byte boundary: the count pass
    reads it byte by byte instead of as 16-byte words."""
    name = f"place[{nops}]"
    h = gc.cases()[name].h
    dev = torch.device("cuda", 0)
    dh = shard.device_history(h, dev)
    buf = torch.zeros(nops + 1, dtype=torch.uint8, device=dev)
    buf[1:] = dh.is_write
    dh.is_write = buf[1:]
    assert dh.is_write.data_ptr() % 16 == 1
    _check_raw(shard.GpuGraph(validator, dev), dh, h.ntxn, _ref(oracle_mod, name, h))


@pytest.mark.parametrize("build", ["host", "device"])
def test_cut_flag_and_scan_path(validator, oracle_mod, build):
    """More valid raw rows than the one-pass cut holds (kCutFastCap = 65536):
    the all-ones cut comes from the flag-and-scan passes, every raw row once;
    under the oracle's own cover, and under a thinned one, the cut is the
    oracle's edges between covered txns."""
    h = gc.big_cut_history()
    r = _ref(oracle_mod, "big_cut", h)
    dev = torch.device("cuda", 0)
    g = shard.GpuGraph(validator, dev)
    rows = _check_raw(g, shard.device_history(h, dev) if build == "device" else h, h.ntxn, r)
    assert len(rows) > 65536
    np.testing.assert_array_equal(np.sort(rows), np.sort(gc.raw_rows(h)))  # duplicates and all
    # (arbitrary observed ids: the backward intervals cover nearly every txn, so a
    # thinned cover -- two txns of three -- makes the cut drop rows as well)
    thin = r.cover & (np.arange(h.ntxn) % 3 != 0)
    for cv in (r.cover, thin):
        cut = _cut_rows(g, torch.from_numpy(cv.astype(np.uint8)).to(dev))
        both = cv[r.s] & cv[r.d]
        assert both.any()
        np.testing.assert_array_equal(np.unique(cut), r.rows[both])
    assert 0 < (thin[r.s] & thin[r.d]).sum() < len(r.s)


def test_builds_reuse_buffers_exactly(validator, oracle_mod):
    """A large build, then a tiny one, then one without ops, on one context:
    nothing of the earlier build (packed writers, backward rows, row counts)
    shows in the later ones."""
    dev = torch.device("cuda", 0)
    g = shard.GpuGraph(validator, dev)
    seq = [("big_cut", gc.big_cut_history())] + [(n, gc.cases()[n].h) for n in ("self_rmw", "empty_5", "one_write",
                                                                               "empty_0")]
    for name, h in seq:
        r = _ref(oracle_mod, name, h)
        _check_raw(g, shard.device_history(h, dev), h.ntxn, r)
        _check_raw(g, h, h.ntxn, r)
        _check_full(validator, h, r)


def test_multi_graph_scc_op_range_cut_rings(oracle_mod):
    """The cut by the covered txns' op ranges (k_cut_txn_ops), reached only
    through hsc_multi_graph_scc: disjoint 3-rings whose membership needs one
    ww row (found by the exact packed search, its source writing the key
    twice), one wr row and one rw row each (test_graph_cases.py shows the
    oracle's answer changes without any one of them), chained acyclic txns
    between them.  Components = Tarjan's, one member and two."""
    h, rings = gc.ring_history()
    r = _ref(oracle_mod, "rings", h)
    assert (np.bincount(r.scc, minlength=h.ntxn) == 3).sum() == len(rings)
    np.testing.assert_array_equal(_multi_scc(h), r.scc)
    np.testing.assert_array_equal(_multi_scc(h, world=2), r.scc)


@pytest.mark.parametrize("n_nodes,m", [(4096, None), (4097, None), (4096, 24576), (4096, 24577)])
def test_scc_cut_one_workgroup_limits(validator, oracle_mod, n_nodes, m):
    """scc_cut runs the SCC in one workgroup up to 4096 cut nodes and 24576
    rows (~0 padding and duplicates counted), past either on the frontier
    kernels: the labels equal Tarjan's on the same rows on both sides of both
    limits; uncovered txns are their own components."""
    ntxn = 6000
    cover, rows, (s, d) = gc.scc_limit_case(n_nodes, m, ntxn=ntxn)
    want = oracle_mod.scc(ntxn, s, d)
    sizes = np.bincount(want, minlength=ntxn)
    assert (sizes == 3).sum() > 100 and (sizes == 4).sum() > 100 and sizes.max() == 4
    valid = rows[rows != -1]
    assert (rows == -1).sum() >= 3 and len(np.unique(valid)) < len(valid)  # padding and duplicates
    dev = torch.device("cuda", 0)
    scc = torch.full((ntxn,), -7, dtype=torch.int32, device=dev)
    st = shard.GpuGraph(validator, dev).scc_cut(ntxn, torch.from_numpy(cover).to(dev), torch.from_numpy(rows).to(dev),
                                                scc)
    assert st["cut_nodes"] == n_nodes and len(rows) == (m or len(rows))
    got = scc.cpu().numpy().astype(np.uint32)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got[cover == 0], np.nonzero(cover == 0)[0])
