"""The host side of the dependency-graph entries (hsc_graph_host.cpp): what
the code they share could get wrong.  The one-call SCC and build + SCC are one
helper and must answer alike; the three build entries end in one tail; every
entry comes in through one preamble; and a refused call must leave the
context's staging and build state as the header says.

The device-error exits (a failed launch or copy) are not provoked here."""
import numpy as np
import pytest
import torch  # imported before any test initialises HIP

import resolve_model as M
import si_model as S
from comdb2_amd import hsc, shard
from comdb2_amd.workloads import History, config4_history, history_window, int64_words, value_history
from test_anomaly import RING4, SERIAL, WRITE_SKEW
from test_anomaly import assert_matches as assert_anomalies
from test_anomaly import ref_of_history as anomalies_ref
from test_gpu_si import assert_matches as assert_si

pytestmark = pytest.mark.gpu

NO_TXNS = History(np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint8), np.zeros(0, np.int64), 0)
HAND = {"write_skew": WRITE_SKEW, "ring4": RING4, "serial": SERIAL, "empty": NO_TXNS}
COUNTS = ("edges", "ww", "wr", "rw", "nontrivial_sccs", "txns_in_cycles", "rounds", "iterations")
EINVAL, EDEVICE, ESTATE = (r"-> %d:" % rc for rc in (hsc.HSC_EINVAL, hsc.HSC_EDEVICE, hsc.HSC_ESTATE))

_GEN = {}


def generated(oracle_mod):
    """3000 txns with cycles, and the oracle's edges and components (once)."""
    if not _GEN:
        h = config4_history(seed=5, n_txn=3000, n_keys=200, concurrent_frac=0.3, max_lag=16)
        _GEN["h"] = h
        _GEN["ref"] = reference(oracle_mod, h)
    return _GEN["h"], _GEN["ref"]


def reference(oracle_mod, h):
    s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
    return s, d, t, oracle_mod.scc(h.ntxn, s, d)


def assert_edges(v, s, d, t):
    for got, want in zip(v.dep_graph_edges(), (s, d, t)):
        np.testing.assert_array_equal(got, want)


# ---- 1. the one-call SCC is build + SCC ------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND) + ["generated"])
def test_one_call_scc_equals_build_then_scc(validator, oracle_mod, name):
    """build_ms: the one call's own, above 0 (the build's sorts and scans are
    launched for the empty history too); exactly 0 from
    dep_graph_scc_built, which builds nothing."""
    h, (s, d, t, want) = generated(oracle_mod) if name == "generated" else (HAND[name], reference(oracle_mod, HAND[name]))
    one, st1 = validator.dep_graph_scc(h)
    one = one.copy()
    validator.dep_graph_build(h, full=True)
    two, st2 = validator.dep_graph_scc_built(h.ntxn)
    np.testing.assert_array_equal(one, want)
    np.testing.assert_array_equal(two, want)
    assert one.dtype == two.dtype == np.uint32 and len(one) == len(two) == h.ntxn
    assert [st1[k] for k in COUNTS] == [st2[k] for k in COUNTS]
    sizes = np.bincount(want, minlength=max(h.ntxn, 1))
    assert [st1[k] for k in COUNTS[:6]] == [len(s)] + [int(((t >> b) & 1).sum()) for b in range(3)] + \
        [int((sizes > 1).sum()), int(sizes[sizes > 1].sum())]
    print(f"{name}: one call build {st1['build_ms']:.4f} ms scc {st1['scc_ms']:.4f} ms; "
          f"built: build {st2['build_ms']} ms scc {st2['scc_ms']:.4f} ms")
    assert st1["build_ms"] > 0 and st2["build_ms"] == 0
    if h.ntxn == 0:
        assert [st1[k] for k in COUNTS] == [0] * len(COUNTS)
    else:
        assert st1["scc_ms"] > 0 and st2["scc_ms"] > 0


# ---- 2. the three build entries ----------------------------------------------------
def test_three_build_entries_agree(validator, oracle_mod):
    h, (s, d, t, _) = generated(oracle_mod)
    dev = torch.device("cuda", 0)
    vh = value_history(h)  # every txn committed
    dh = shard.device_history(h, dev)
    hs, keep = validator._history(h)
    lib, ctx = validator.lib, validator.ctx

    def resolved():
        res = validator.dep_graph_resolve(vh, arrays=False)
        assert res["ncommitted"] == h.ntxn and res["dropped"] == 0
        return validator.dep_graph_build_resolved(full=True)

    # with the stats, and without (a null st: the build alone, rc 0)
    entries = {
        "host": (lambda: validator.dep_graph_build(h, full=True),
                 lambda: lib.hsc_dep_graph_build(ctx, hsc.C.byref(hs), 1, None)),
        "device": (lambda: shard.GpuGraph(validator, dev, full=True).build(dh),
                   lambda: lib.hsc_dep_graph_build_device(ctx, dh.nops, dh.ntxn, dh.txn.data_ptr(), dh.key.data_ptr(),
                                                          dh.is_write.data_ptr(), dh.observed.data_ptr(), 1, None)),
        "resolved": (resolved, lambda: lib.hsc_dep_graph_build_resolved(ctx, 1, None)),
    }
    want = [len(s)] + [int(((t >> b) & 1).sum()) for b in range(3)]
    for name, (with_st, without_st) in entries.items():
        st = with_st()
        assert [st[k] for k in ("edges", "ww", "wr", "rw")] == want, name
        assert st["build_ms"] > 0 and st["scc_ms"] == 0, name
        assert_edges(validator, s, d, t)
        validator.dep_graph_build(NO_TXNS, full=True)  # another graph in between
        assert without_st() == hsc.HSC_OK, name
        assert_edges(validator, s, d, t)


# ---- 3. refused calls -----------------------------------------------------------------
def test_refused_calls_leave_the_context_usable(oracle_mod):
    h, (s, d, t, _) = generated(oracle_mod)
    hw = history_window(h)
    ids = np.arange(h.ntxn)
    dev = torch.device("cuda", 0)
    v = hsc.Validator(0)
    try:
        # a raw build has no CSR for the passes over a full one
        v.dep_graph_build(h, full=False)
        for call in (lambda: v.dep_graph_scc_built(h.ntxn), v.dep_graph_anomalies, v.dep_graph_si):
            with pytest.raises(hsc.HscError, match=ESTATE):
                call()
        # a txn completing before its invoke: nothing staged, not even what was
        inv = 2 * ids.astype(np.uint64)
        assert v.dep_graph_stage_realtime(inv, inv + np.uint64(1))["edges"] > 0
        bad = inv.copy()
        bad[17] = inv[17] + np.uint64(2)
        with pytest.raises(hsc.HscError, match=EINVAL):
            v.dep_graph_stage_realtime(bad, inv + np.uint64(1))
        v.dep_graph_build(h, full=True)
        assert not (v.dep_graph_edges()[2] & 8).any()
        assert_edges(v, s, d, t)
        # a staged rw pair that names a txn the build does not have
        v.register_group("t1", 0, 9)
        gid = torch.zeros(len(hw.keys), dtype=torch.int32, device=dev)
        words = torch.from_numpy(int64_words(hw.keys).reshape(-1).view(np.int64)).to(dev)
        lsn = torch.from_numpy(hw.lsn.view(np.int64)).to(dev)
        v.ingest_device(len(hw.keys), 2, gid.data_ptr(), words.data_ptr(), lsn.data_ptr(), hw.end_lsn)
        torch.cuda.synchronize()
        assert len(v.rw_edges(hw.readsets)[0]) > 0
        past = ids.copy()
        past[-1] = h.ntxn
        v.dep_graph_stage_rw_pairs(ids, hw.commit_lsn, past)
        with pytest.raises(hsc.HscError, match=EINVAL):
            v.dep_graph_build(h, full=True, no_rw=True)
        v.dep_graph_build(h, full=True, no_rw=True)  # the staged rows are gone: ww and wr only
        own = (t & 3) != 0
        assert_edges(v, s[own], d[own], t[own] & 3)
        # a cut row with an endpoint outside the cover
        cover = torch.tensor([1, 1, 0, 1], dtype=torch.uint8, device=dev)
        rows = torch.tensor([(0 << 32) | 2], dtype=torch.int64, device=dev)
        with pytest.raises(hsc.HscError, match=EINVAL):
            shard.GpuGraph(v, dev).scc_cut(4, cover, rows, torch.empty(4, dtype=torch.int32, device=dev))
        # an invalid value history resolves to nothing
        for name in sorted(M.INVALID):
            with pytest.raises(hsc.HscError, match="hsc_dep_graph_resolve " + EINVAL):
                v.dep_graph_resolve(M.INVALID[name])
            with pytest.raises(hsc.HscError, match="hsc_dep_graph_build_resolved " + ESTATE):
                v.dep_graph_build_resolved()
        # and the context goes on answering
        ws, wd, wt, wscc = reference(oracle_mod, WRITE_SKEW)
        scc, st = v.dep_graph_scc(WRITE_SKEW)
        np.testing.assert_array_equal(scc, wscc)
        assert_edges(v, ws, wd, wt)
        assert st["build_ms"] > 0 and st["scc_ms"] > 0
        an = v.dep_graph_anomalies()
        assert_anomalies(an, anomalies_ref(oracle_mod, WRITE_SKEW), WRITE_SKEW.ntxn)
        si = v.dep_graph_si()
        assert_si(si, S.ref_of_history(oracle_mod, WRITE_SKEW), WRITE_SKEW.ntxn)
        g1b = M.HAND["g1b"][0]
        res = v.dep_graph_resolve(g1b)
        M.assert_equal(res, M.resolve(g1b))
        assert an["ms"] > 0 and si["ms"] > 0 and res["ms"] > 0
    finally:
        v.close()


# ---- 4. a context without a device ---------------------------------------------------
def test_host_only_context_refuses_every_graph_entry():
    none = np.zeros(0, np.uint64)
    v = hsc.Validator(-1)
    try:
        entries = {
            "scc": lambda: v.dep_graph_scc(WRITE_SKEW),
            "build": lambda: v.dep_graph_build(WRITE_SKEW, full=True),
            "build_device": lambda: v.dep_graph_build_device(0, 0, 0, 0, 0, 0, full=True),
            "resolve": lambda: v.dep_graph_resolve(M.HAND["g1a"][0]),
            "build_resolved": v.dep_graph_build_resolved,
            "stage_rw_pairs": lambda: v.dep_graph_stage_rw_pairs(none, none, none),
            "stage_realtime": lambda: v.dep_graph_stage_realtime(none, none),
            "scc_built": lambda: v.dep_graph_scc_built(0),
            "anomalies": v.dep_graph_anomalies,
            "si": v.dep_graph_si,
            "cover": lambda: v.dep_graph_cover(0),
            "cut": lambda: v.dep_graph_cut(0),
            "scc_cut": lambda: v.dep_graph_scc_cut(0, 0, 0, 0, 0),
            "edges": v.dep_graph_edges,
        }
        assert sorted("dep_graph_" + k for k in entries) == sorted(k for k in dir(v) if k.startswith("dep_graph_"))
        for name, call in entries.items():
            with pytest.raises(hsc.HscError, match="hsc_dep_graph_%s %s" % (name, EDEVICE)):
                call()
        with pytest.raises(hsc.HscError, match="hsc_dep_graph_build %s host-only context" % EDEVICE):
            v.dep_graph_build(WRITE_SKEW)
    finally:
        v.close()
