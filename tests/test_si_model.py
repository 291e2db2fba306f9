"""Snapshot isolation from the dependency graph (hsc_dep_graph_si, DESIGN.md
§5f): the CPU reference (si_model.py) against the statement read literally,
the hand-built histories, the implication from §5d's classes, the ABI and the
Jepsen report's pure part.  The GPU side is tests/test_gpu_si.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

import si_model as S
from comdb2_amd import hsc
from comdb2_amd import jepsen as J
from test_anomaly import (G1C, G2, GSINGLE, MUTUAL, READ_SKEW, RING4, SERIAL, WRITE_SKEW, generated, hist,
                          ref_anomalies)

# 0 -wr-> 1 -rw-> 2 -wr-> 3 -rw-> 0: two anti edges, not adjacent
NONADJ4_ROWS = [(0, 1, "w"), (0, 4, "w"), (1, 1, "r", 0), (1, 2, "r", -1), (2, 2, "w"), (2, 3, "w"),
                (3, 3, "r", 2), (3, 4, "r", -1)]
NONADJ4 = hist(NONADJ4_ROWS, 4)
# txn 4 tied to txn 0 by a write-skew 2-cycle only
PARTIAL5 = hist(NONADJ4_ROWS + [(4, 4, "r", -1), (0, 5, "r", -1), (4, 5, "w")], 5)
SI_HAND = {"write_skew": WRITE_SKEW, "ring4": RING4, "read_skew": READ_SKEW, "mutual": MUTUAL,
           "serial": SERIAL, "nonadj4": NONADJ4, "partial5": PARTIAL5}
SI_HAND_BITS = {"write_skew": [0, 0], "ring4": [0] * 4, "read_skew": [1, 1], "mutual": [1, 1],
                "serial": [0, 0, 0], "nonadj4": [1] * 4, "partial5": [1, 1, 1, 1, 0]}

_REFS = {}


def refs_for(oracle_mod, name):
    """(ref_si, ref_anomalies) of a generated history, computed once."""
    if name not in _REFS:
        h = generated(name)
        s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
        _REFS[name] = (S.ref_si(oracle_mod, h.ntxn, s, d, t), ref_anomalies(oracle_mod, h.ntxn, s, d, t))
    return _REFS[name]


def both_refs(oracle_mod, h):
    s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
    return S.ref_si(oracle_mod, h.ntxn, s, d, t), ref_anomalies(oracle_mod, h.ntxn, s, d, t)


def random_typed_graph(rng):
    n = int(rng.integers(2, 8))
    m = int(rng.integers(1, 3 * n + 1))
    edges = {}
    for _ in range(m):
        u, v = int(rng.integers(0, n)), int(rng.integers(0, n))
        if u != v:
            edges[(u, v)] = int(rng.choice([1, 2, 4, 6, 8, 12]))
    return n, edges


def test_literal_model_on_random_typed_graphs(oracle_mod):
    """Per component: a simple cycle without adjacent anti edges exists <=>
    comp_nonadj.  Per txn: on such a simple cycle => nonadj (the bit speaks of
    closed walks).  And the reduction of a BFS walk in P always ends in a
    simple good cycle through txns that carry the bit."""
    rng = np.random.default_rng(20240)
    seen = {"flagged": 0, "legal": 0, "walk_longer": 0, "bit_off_cycle": 0}
    for _ in range(3000):
        n, edges = random_typed_graph(rng)
        keys = sorted(edges)
        s = np.array([k[0] for k in keys], np.int64)
        d = np.array([k[1] for k in keys], np.int64)
        t = np.array([edges[k] for k in keys], np.int64)
        r = S.ref_si(oracle_mod, n, s, d, t)
        lit = S.literal_good_nodes(n, edges)
        assert all(r.nonadj[v] for v in lit)
        seen["bit_off_cycle"] += int(r.nonadj.sum()) > len(lit)
        for lab, f in zip(r.comp_label.tolist(), r.comp_nonadj.tolist()):
            members = set(np.nonzero(r.scc == lab)[0].tolist())
            assert bool(f) == bool(lit & members)
            seen["flagged" if f else "legal"] += 1
        for (a, b) in keys:
            w = S.product_walk(edges, a, b)
            inside = r.scc[a] == r.scc[b]
            lifts = [(2 * a + k, 2 * b + (edges[(a, b)] == 4)) for k in ((0,) if edges[(a, b)] == 4 else (0, 1))]
            on_p_cycle = inside and any(r.pscc[x] == r.pscc[y] for x, y in lifts)
            assert (w is not None) == bool(on_p_cycle)
            if w is None:
                continue
            assert S.good_cycle(w[1])
            tx, ty = S.reduce_walk(*w)
            seen["walk_longer"] += len(w[0]) > len(tx)
            assert len(tx) >= 2 and len(set(tx)) == len(tx) and S.good_cycle(ty)
            assert all(edges[(tx[i], tx[(i + 1) % len(tx)])] == ty[i] for i in range(len(tx)))
            assert all(r.nonadj[v] for v in tx) and len({int(r.scc[v]) for v in tx}) == 1
    # the draw covers every outcome
    assert all(v > 0 for v in seen.values()), seen


@pytest.mark.parametrize("name", sorted(SI_HAND))
def test_reference_hand_built(oracle_mod, name):
    h = SI_HAND[name]
    r, a = both_refs(oracle_mod, h)
    assert r.nonadj.tolist() == SI_HAND_BITS[name]
    if name in ("write_skew", "ring4"):
        assert a.comp_class.tolist() == [G2] and r.comp_nonadj.tolist() == [0] and r.comps == 0
    elif name == "serial":
        assert len(r.comp_label) == 0 and r.core_nodes == 0 and r.product_edges == 0
    else:
        assert r.comp_nonadj.tolist() == [1] and r.comps == 1
    if name == "nonadj4":
        assert list(zip(r.s.tolist(), r.d.tolist(), r.t.tolist())) == [(0, 1, 2), (1, 2, 4), (2, 3, 2), (3, 0, 4)]
        assert a.cls.tolist() == [4, 4, 4, 4]  # G2 only: the class the plain analysis cannot tell apart
    if name == "partial5":
        assert len(r.comp_label) == 1 and a.comp_class.tolist() == [G2] and r.txns == 4
    np.testing.assert_array_equal(r.comp_label, a.comp_label)


@pytest.mark.parametrize("name", ["mixed3000", "skew1500_0", "skew1500_1"])
def test_classes_imply_the_bit(oracle_mod, name):
    r, a = refs_for(oracle_mod, name)
    np.testing.assert_array_equal(r.comp_label, a.comp_label)
    assert not (((a.cls & (G1C | GSINGLE)) != 0) & (r.nonadj == 0)).any()
    assert r.core_nodes == a.core_nodes
    by_class = {k: r.comp_nonadj[a.comp_class == k] for k in (G1C, GSINGLE, G2)}
    assert by_class[G1C].all() and by_class[GSINGLE].all()
    g2_flagged, g2_legal = int(by_class[G2].sum()), int((by_class[G2] == 0).sum())
    print(name, "comps", a.comps, "nonadjacent", r.comps, "txns", r.txns, "G2 flagged / legal", g2_flagged, g2_legal)
    if name == "mixed3000":
        # the input keeps a G2 component of each kind
        assert g2_flagged >= 1 and g2_legal >= 1
        assert (a.comps, r.comps, r.txns, r.core_nodes) == ([10, 3, 3], 15, 2162, 2184)
        g2 = a.comp_label[a.comp_class == G2].tolist()
        assert dict(zip(g2, by_class[G2].tolist())) == {92: 0, 2052: 1, 2627: 1}
        sizes = {lab: int((r.scc == lab).sum()) for lab in g2}
        assert sizes == {92: 9, 2052: 9, 2627: 7}
        partial = sum(1 for lab, f in zip(r.comp_label.tolist(), r.comp_nonadj.tolist())
                      if f and not r.nonadj[r.scc == lab].all())
        assert partial == 4
    else:
        assert a.comps == ([0, 56, 4] if name.endswith("0") else [0, 59, 2])
        assert g2_flagged == 0 and r.comps == a.comps[1]
        assert r.txns == (122 if name.endswith("0") else 128)


def test_jepsen_generated_verdicts(oracle_mod):
    """adya.clj's write skew is legal under snapshot isolation; the register
    histories' read skew is not."""
    for seed, want in zip(range(3), (25, 25, 19)):
        h = J.history_from_jepsen_edn(J.adya_g2_edn(seed)[0]).history
        r, a = both_refs(oracle_mod, h)
        assert a.comps == [0, 0, want] and r.comps == 0 and r.txns == 0
    for seed, want in zip(range(3), (8, 4, 16)):
        h = J.history_from_jepsen_edn(J.register_history_edn(seed)[0]).history
        r, a = both_refs(oracle_mod, h)
        assert a.comps == [0, want, 0] and r.comps == want and r.comp_nonadj.all()


def test_abi_entry_point():
    lib = hsc.load()
    assert hasattr(lib, "hsc_dep_graph_si")
    assert "hsc_dep_graph_si" in hsc.EXPORTS
    out = hsc.SiReport()
    assert lib.hsc_dep_graph_si(None, 0, ctypes.byref(out)) == hsc.HSC_EINVAL
    v = hsc.Validator(-1)  # host-only
    try:
        assert lib.hsc_dep_graph_si(v.ctx, 0, None) == hsc.HSC_EINVAL
        assert lib.hsc_dep_graph_si(v.ctx, 0, ctypes.byref(out)) == hsc.HSC_EDEVICE
        with pytest.raises(hsc.HscError):
            v.dep_graph_si()
    finally:
        v.close()


def test_struct_layout_matches_header(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    fields = [f for f, _ in hsc.SiReport._fields_]
    prog = tmp_path / "layout.c"
    prog.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"hip_serial.h\"\n"
                    "int main(void){printf(\"%zu %d\", sizeof(hsc_si_report), HSC_SI_WITNESS);\n"
                    + "".join(f"printf(\" %zu\", offsetof(hsc_si_report, {f}));\n" for f in fields)
                    + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    R = hsc.SiReport
    assert got == [ctypes.sizeof(R), hsc.SI_WITNESS] + [getattr(R, f).offset for f in fields]
    assert ctypes.sizeof(R) == 104


class _Ops:
    txn_ops = [{":n": i} for i in range(8)]


def test_isolation_report_is_a_pure_function():
    u8, u32 = (lambda x: np.array(x, np.uint8)), (lambda x: np.array(x, np.uint32))
    result = {"comp_label": u32([1, 4, 7]), "comp_class": u8([4, 2, 4]), "txns": [0, 2, 7]}
    si = {"comp_label": u32([1, 4, 7]), "comp_nonadj": u8([0, 1, 1]), "wit_off": u32([0, 0, 2, 6]),
          "wit_txn": u32([3, 4, 2, 5, 6, 7]), "wit_type": u8([2, 4, 2, 4, 10, 4])}
    rep = J.isolation_report(_Ops, result, si)
    assert rep["snapshot_isolation_valid"] is False
    assert rep["levels"] == {"g1c_free": True, "snapshot_isolation": False, "serializable": False}
    assert [c["type"] for c in rep["si_cycles"]] == ["G-single", "G-nonadjacent"]
    assert [c["label"] for c in rep["si_cycles"]] == [4, 7]
    assert rep["si_cycles"][0]["txns"] == [3, 4] and rep["si_cycles"][0]["edge_types"] == ["wr", "rw"]
    assert rep["si_cycles"][1]["edge_types"] == ["wr", "rw", "wr+rt", "rw"]
    assert rep["si_cycles"][1]["ops"] == [_Ops.txn_ops[t] for t in (2, 5, 6, 7)]
    # write skew only: not serializable, snapshot isolation holds
    legal = dict(si, comp_nonadj=u8([0, 0, 0]), wit_off=u32([0, 0, 0, 0]), wit_txn=u32([]), wit_type=u8([]))
    rep = J.isolation_report(_Ops, result, legal)
    assert rep["snapshot_isolation_valid"] is True and rep["si_cycles"] == []
    assert rep["levels"] == {"g1c_free": True, "snapshot_isolation": True, "serializable": False}
    # without witnesses the cycles are listed, empty
    bare = dict(si, wit_off=u32([0, 0, 0, 0]), wit_txn=u32([]), wit_type=u8([]))
    assert [c["txns"] for c in J.isolation_report(_Ops, result, bare)["si_cycles"]] == [[], []]
    # the real-time pass adds its two levels; G1c shows in g1c_free
    none = {"comp_label": u32([]), "comp_class": u8([]), "txns": [0, 0, 0]}
    si_none = {"comp_label": u32([]), "comp_nonadj": u8([]), "wit_off": u32([0]), "wit_txn": u32([]),
               "wit_type": u8([])}
    strict = {"comp_label": u32([2]), "comp_class": u8([2]), "txns": [0, 2, 2]}
    strict_si = {"comp_label": u32([2]), "comp_nonadj": u8([1])}
    rep = J.isolation_report(_Ops, none, si_none, strict, strict_si)
    assert rep["levels"] == {"g1c_free": True, "snapshot_isolation": True, "serializable": True,
                             "strict_serializable": False, "strong_snapshot_isolation": False}
    assert "strong_snapshot_isolation" not in J.isolation_report(_Ops, none, si_none, strict)["levels"]
    g1c = {"comp_label": u32([1]), "comp_class": u8([1]), "txns": [2, 0, 0]}
    assert J.isolation_report(_Ops, g1c, dict(si_none, comp_label=u32([1]), comp_nonadj=u8([1]),
                                              wit_off=u32([0, 0])))["levels"]["g1c_free"] is False
