"""Which anomaly a dependency cycle is (G1c / G-single / G2) and its witness
cycle: hsc_dep_graph_anomalies (include/hip_serial.h).

The reference below restates the definitions on the CPU from the oracle's
edges (oracle_mod.dep_edges) and Tarjan (oracle_mod.scc) alone:

* E1 = edges with type & 3; an anti edge has type == 4 exactly;
* bit 1 (G1c): the txn's component of (V, E1) has >= 2 txns -- E1 cut down to
  the edges inside a full component first (an E1 cycle lies inside one);
* bit 4 (G2): the txn's full component has >= 2 txns and an anti edge inside;
* bit 2 (G-single): an anti edge a -> b inside the component with b ~> v ~> a
  over E1 edges inside it: E1 condensed by its components, one Python-int
  bit set per condensed node (bit j = anti edge j), F carried in topological
  order and B against it.

The GPU results (-m gpu) must equal it exactly; every witness is checked
against the edges and against a plain BFS for its length."""
import ctypes
import functools
from collections import deque

import numpy as np
import pytest
import torch  # noqa: F401  (imported before any test initialises HIP)

from comdb2_amd import hsc
from comdb2_amd.workloads import History, config4_history

G1C, GSINGLE, G2 = 1, 2, 4


def hist(rows, ntxn):
    """rows: (txn, key, 'r'|'w'[, observed writer or -1])."""
    rows = [r if len(r) == 4 else r + (-1,) for r in rows]
    t, k, w, o = zip(*rows)
    return History(np.array(t, np.uint32), np.array(k, np.uint64),
                   np.array([x == "w" for x in w], np.uint8), np.array(o, np.int64), ntxn)


def with_future_reads(h, frac, seed):
    """Reads that saw a version committed after their own txn: walking the
    reads in op order, one draw each; a draw < frac moves the read's observed
    version to the key's first writer with a larger txn id (if any)."""
    rng = np.random.default_rng(seed)
    writers = {}
    for k in np.unique(h.key[h.is_write != 0]):
        writers[int(k)] = np.unique(h.txn[(h.is_write != 0) & (h.key == k)])
    obs = h.observed.copy()
    for i in np.nonzero(h.is_write == 0)[0]:
        if rng.random() >= frac:
            continue
        ws = writers.get(int(h.key[i]))
        if ws is None:
            continue
        j = int(np.searchsorted(ws, h.txn[i], side="right"))
        if j < len(ws):
            obs[i] = int(ws[j])
    return History(h.txn, h.key, h.is_write, obs, h.ntxn)


# ---------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------
class Ref:
    """cls[ntxn], comp_label / comp_class, the stats, and per anti edge
    inside a component whether it is closed (closed_idx: their edge indices)."""


def _lowest_bit(x):
    return x & -x


def ref_anomalies(oracle_mod, ntxn, s, d, t):
    r = Ref()
    s, d, t = (np.asarray(x, np.int64) for x in (s, d, t))
    r.s, r.d, r.t = s, d, t
    scc = oracle_mod.scc(ntxn, s, d).astype(np.int64) if ntxn else np.zeros(0, np.int64)
    r.scc = scc
    nontriv = np.bincount(scc, minlength=ntxn)[scc] > 1 if ntxn else np.zeros(0, bool)
    inside = scc[s] == scc[d]
    r.inside = inside
    e1 = inside & ((t & 3) != 0)
    anti = inside & (t == 4)
    scc1 = oracle_mod.scc(ntxn, s[e1], d[e1]).astype(np.int64) if ntxn else scc
    r.scc1 = scc1
    cls = np.zeros(ntxn, np.uint8)
    if ntxn:
        cls[np.bincount(scc1, minlength=ntxn)[scc1] > 1] |= G1C
        has_anti = np.zeros(ntxn, bool)
        has_anti[scc[s[anti]]] = True
        cls[has_anti[scc] & nontriv] |= G2
    r.anti_idx = np.nonzero(anti)[0]
    r.anti_edges = int(anti.sum())
    # E1 inside the components, condensed: node ids = dense ranks of scc1 over the core
    core = np.nonzero(nontriv)[0]
    labs, cond_of_core = np.unique(scc1[core], return_inverse=True)
    cond = np.full(ntxn, -1, np.int64)
    cond[core] = cond_of_core
    n = len(labs)
    cu, cw = cond[s[e1]], cond[d[e1]]
    keep = cu != cw
    pairs = np.unique(np.stack([cu[keep], cw[keep]], 1), axis=0) if keep.any() else np.zeros((0, 2), np.int64)
    succ = [[] for _ in range(n)]
    indeg = [0] * n
    for u, w in pairs.tolist():
        succ[u].append(w)
        indeg[w] += 1
    order = [u for u in range(n) if indeg[u] == 0]
    for u in order:  # Kahn (order grows while it is walked)
        for w in succ[u]:
            indeg[w] -= 1
            if indeg[w] == 0:
                order.append(w)
    assert len(order) == n
    F, B = [0] * n, [0] * n
    aa, ab = cond[s[r.anti_idx]].tolist(), cond[d[r.anti_idx]].tolist()
    for j, (a, b) in enumerate(zip(aa, ab)):
        F[b] |= 1 << j
        B[a] |= 1 << j
    for u in order:
        fu = F[u]
        if fu:
            for w in succ[u]:
                F[w] |= fu
    for u in reversed(order):
        bu = B[u]
        for w in succ[u]:
            bu |= B[w]
        B[u] = bu
    hit = np.array([(F[u] & B[u]) != 0 for u in range(n)], bool)
    if n:
        cls[core[hit[cond_of_core]]] |= GSINGLE
    closed = np.array([(F[a] >> j) & 1 for j, a in enumerate(aa)], bool)
    r.closed_idx = r.anti_idx[closed] if len(aa) else r.anti_idx
    r.cls = cls
    r.comp_label = np.unique(scc[nontriv]).astype(np.uint32) if ntxn else np.zeros(0, np.uint32)
    cor = np.zeros(ntxn, np.uint8)
    if ntxn:
        np.bitwise_or.at(cor, scc, cls)
    r.comp_class = np.array([_lowest_bit(int(cor[c])) for c in r.comp_label], np.uint8)
    r.comps = [int((r.comp_class == k).sum()) for k in (G1C, GSINGLE, G2)]
    r.txns = [int(((cls & k) != 0).sum()) for k in (G1C, GSINGLE, G2)]
    r.core_nodes = int(nontriv.sum())
    return r


def ref_of_history(oracle_mod, h):
    s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
    return ref_anomalies(oracle_mod, h.ntxn, s, d, t)


def check_witnesses(res, ref):
    """Every property the header promises of a witness."""
    s, d, t, scc = ref.s, ref.d, ref.t, ref.scc
    ins = np.nonzero(ref.inside)[0]
    edge = {(int(s[i]), int(d[i])): i for i in ins.tolist()}
    adj = {}
    for i in ins.tolist():
        adj.setdefault(int(s[i]), []).append((int(d[i]), int(t[i])))
    off = res["wit_off"]
    assert len(off) == len(res["comp_label"]) + 1 and off[0] == 0
    assert off[-1] == len(res["wit_txn"]) == len(res["wit_type"])
    closed = set(ref.closed_idx.tolist())
    for c, (lab, k) in enumerate(zip(res["comp_label"].tolist(), res["comp_class"].tolist())):
        tx = res["wit_txn"][off[c]:off[c + 1]].tolist()
        ty = res["wit_type"][off[c]:off[c + 1]].tolist()
        assert len(tx) >= 2 and len(set(tx)) == len(tx)
        assert all(scc[v] == lab for v in tx)
        idx = []
        for i, v in enumerate(tx):
            e = edge.get((v, tx[(i + 1) % len(tx)]))
            assert e is not None, "witness step is not an edge of the component"
            assert int(t[e]) == ty[i]
            idx.append(e)
        n_anti = sum(1 for x in ty if x == 4)
        assert (n_anti == 0) if k == G1C else (n_anti == 1) if k == GSINGLE else (n_anti >= 2)
        if k != G2:
            assert all(x & 3 for x in ty[:-1])
        # the closing edge: the lowest qualifying edge of the component
        mine = ins[scc[s[ins]] == lab]
        if k == G1C:
            q = mine[((t[mine] & 3) != 0) & (ref.scc1[s[mine]] == ref.scc1[d[mine]])]
        elif k == G2:
            q = mine[t[mine] == 4]
        else:
            q = np.array([i for i in mine.tolist() if i in closed], np.int64)
        assert len(q) and idx[-1] == int(q.min())
        # shortest: a BFS first ~> last over the class's edges
        mask = 7 if k == G2 else 3
        dist = {tx[0]: 0}
        todo = deque([tx[0]])
        while todo and tx[-1] not in dist:
            u = todo.popleft()
            for w, ty_ in adj.get(u, ()):
                if (ty_ & mask) and w not in dist:
                    dist[w] = dist[u] + 1
                    todo.append(w)
        assert dist[tx[-1]] + 1 == len(tx)


# ---------------------------------------------------------------------------
# histories
# ---------------------------------------------------------------------------
WRITE_SKEW = hist([(0, 1, "r"), (0, 2, "w"), (1, 2, "r"), (1, 1, "w")], 2)
READ_SKEW = hist([(0, 1, "w"), (0, 2, "w"), (1, 1, "r", -1), (1, 2, "r", 0)], 2)
MUTUAL = hist([(0, 1, "w"), (0, 2, "r", 1), (1, 2, "w"), (1, 1, "r", 0)], 2)
RING4 = hist([(i, i, "r") for i in range(4)] + [(i, (i + 1) % 4, "w") for i in range(4)], 4)
SERIAL = hist([(0, 1, "w"), (1, 1, "r", 0), (1, 1, "w"), (2, 1, "r", 1)], 3)
HAND = {"write_skew": WRITE_SKEW, "read_skew": READ_SKEW, "mutual": MUTUAL, "ring4": RING4,
        "serial": SERIAL}


def fan(k):
    """Txn 0 writes x and y_1..y_k; txn i reads y_i at its initial version
    (rw i -> 0) and x from txn 0 (wr 0 -> i): one component, k closed anti
    edges."""
    rows = [(0, 0, "w")] + [(0, i, "w") for i in range(1, k + 1)]
    for i in range(1, k + 1):
        rows += [(i, i, "r", -1), (i, 0, "r", 0)]
    return hist(rows, k + 1)


@functools.lru_cache(maxsize=None)
def generated(name):
    if name == "mixed3000":
        h = config4_history(seed=0, n_txn=3000, n_keys=200, concurrent_frac=0.05, max_lag=8)
        return with_future_reads(h, 0.01, 0)
    if name in ("skew1500_0", "skew1500_1"):
        return config4_history(seed=int(name[-1]), n_txn=1500, n_keys=60, concurrent_frac=0.2, max_lag=6)
    if name == "large":
        h = config4_history(seed=0, n_txn=20000, n_keys=4000, concurrent_frac=0.05, max_lag=16)
        return with_future_reads(h, 0.003, 0)
    raise KeyError(name)


_REFS = {}


def ref_for(oracle_mod, name, h):
    if name not in _REFS:
        _REFS[name] = ref_of_history(oracle_mod, h)
    return _REFS[name]


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_reference_hand_built(oracle_mod):
    r = ref_of_history(oracle_mod, WRITE_SKEW)
    assert r.cls.tolist() == [4, 4] and r.comp_class.tolist() == [G2] and r.comp_label.tolist() == [1]
    r = ref_of_history(oracle_mod, READ_SKEW)
    assert all(c & GSINGLE and not c & G1C for c in r.cls.tolist())
    assert r.comp_class.tolist() == [GSINGLE]
    r = ref_of_history(oracle_mod, MUTUAL)
    assert r.cls.tolist() == [1, 1] and r.comp_class.tolist() == [G1C]
    r = ref_of_history(oracle_mod, RING4)
    assert r.comp_class.tolist() == [G2] and r.anti_edges == 4 and r.cls.tolist() == [4] * 4
    r = ref_of_history(oracle_mod, SERIAL)
    assert not r.cls.any() and len(r.comp_label) == 0 and r.core_nodes == 0


def test_reference_fan(oracle_mod):
    for k in (1, 65):
        r = ref_of_history(oracle_mod, fan(k))
        assert r.cls.tolist() == [GSINGLE | G2] * (k + 1)
        assert r.anti_edges == k == len(r.closed_idx)


def test_reference_gsingle_matches_plain_bfs(oracle_mod):
    """The bit-set reference against the definition read literally: a BFS per
    anti edge (a small history: the literal form is slow)."""
    h = with_future_reads(config4_history(seed=3, n_txn=400, n_keys=30, concurrent_frac=0.2, max_lag=6),
                          0.02, 3)
    r = ref_of_history(oracle_mod, h)
    s, d, t, scc = r.s, r.d, r.t, r.scc
    e1 = r.inside & ((t & 3) != 0)
    fw, bw = {}, {}
    for a, b in zip(s[e1].tolist(), d[e1].tolist()):
        fw.setdefault(a, []).append(b)
        bw.setdefault(b, []).append(a)

    def reach(adj, v):
        seen, todo = {v}, [v]
        while todo:
            for w in adj.get(todo.pop(), ()):
                if w not in seen:
                    seen.add(w)
                    todo.append(w)
        return seen

    want = np.zeros(h.ntxn, bool)
    closed = 0
    for i in r.anti_idx.tolist():
        a, b = int(s[i]), int(d[i])
        both = reach(fw, b) & reach(bw, a)
        closed += a in both
        want[list(both)] = True
    assert r.anti_edges > 0 and closed == len(r.closed_idx)
    np.testing.assert_array_equal((r.cls & GSINGLE) != 0, want)


def test_reference_classes_on_generated_histories(oracle_mod):
    """Every class the histories are meant to hold is there.  (The mixed
    history: 10 G1c, 3 G-single and 3 G2 components, 2184 txns in cycles,
    3290 anti edges inside components of which 1759 are closed.)"""
    r = ref_for(oracle_mod, "mixed3000", generated("mixed3000"))
    print("mixed3000", r.comps, r.txns, r.core_nodes, r.anti_edges, len(r.closed_idx))
    assert all(n > 0 for n in r.comps)
    assert 0 < len(r.closed_idx) < r.anti_edges
    assert (r.comps, r.core_nodes, r.anti_edges, len(r.closed_idx)) == ([10, 3, 3], 2184, 3290, 1759)
    for name in ("skew1500_0", "skew1500_1"):
        r = ref_for(oracle_mod, name, generated(name))
        print(name, r.comps, r.txns, r.core_nodes, r.anti_edges, len(r.closed_idx))
        assert r.comps[0] == 0 and r.comps[1] > 0 and r.comps[2] > 0
        assert r.txns[0] == 0
        assert r.comps == ([0, 56, 4] if name.endswith("0") else [0, 59, 2])


def test_abi_entry_point():
    lib = hsc.load()
    assert hasattr(lib, "hsc_dep_graph_anomalies")
    assert "hsc_dep_graph_anomalies" in hsc.EXPORTS
    # hsc_anomalies on LP64: 2 x (u32 + pad, ptr), 4 ptrs, 6 u32, 2 u64, 4 u32, float + pad
    assert ctypes.sizeof(hsc.Anomalies) == 128
    assert hsc.Anomalies.anti_edges.offset == 88 and hsc.Anomalies.ms.offset == 120
    out = hsc.Anomalies()
    assert lib.hsc_dep_graph_anomalies(None, 0, 0, ctypes.byref(out)) == hsc.HSC_EINVAL
    v = hsc.Validator(-1)  # host-only
    try:
        assert lib.hsc_dep_graph_anomalies(v.ctx, 0, 0, None) == hsc.HSC_EINVAL
        assert lib.hsc_dep_graph_anomalies(v.ctx, 0, 0, ctypes.byref(out)) == hsc.HSC_EDEVICE
        with pytest.raises(hsc.HscError):
            v.dep_graph_anomalies()
    finally:
        v.close()


def test_struct_layout_matches_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = tmp_path / "layout.c"
    prog.write_text("""#include <stdio.h>
#include <stddef.h>
#include "hip_serial.h"
int main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(hsc_anomalies),
 offsetof(hsc_anomalies, comp_class), offsetof(hsc_anomalies, comps), offsetof(hsc_anomalies, anti_edges),
 offsetof(hsc_anomalies, ms), HSC_ANOM_G1C, HSC_ANOM_GSINGLE, HSC_ANOM_G2, HSC_ANOM_WITNESS); return 0;}""")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(prog), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True,
                                          check=True).stdout.split()]
    A = hsc.Anomalies
    assert got == [ctypes.sizeof(A), A.comp_class.offset, A.comps.offset, A.anti_edges.offset,
                   A.ms.offset, hsc.ANOM_G1C, hsc.ANOM_GSINGLE, hsc.ANOM_G2, hsc.ANOM_WITNESS]


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def analyse(validator, h, **kw):
    validator.dep_graph_build(h, full=True)
    return validator.dep_graph_anomalies(**kw)


def assert_matches(res, ref, ntxn):
    assert len(res["cls"]) == ntxn
    np.testing.assert_array_equal(res["cls"], ref.cls)
    np.testing.assert_array_equal(res["comp_label"], ref.comp_label)
    np.testing.assert_array_equal(res["comp_class"], ref.comp_class)
    assert res["comps"] == ref.comps and res["txns"] == ref.txns
    assert res["core_nodes"] == ref.core_nodes
    assert res["anti_edges"] == res["anti_tested"] == ref.anti_edges
    assert res["reach_batches"] == (ref.anti_edges + 63) // 64


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(HAND))
def test_gpu_hand_built(validator, oracle_mod, name):
    h = HAND[name]
    ref = ref_of_history(oracle_mod, h)
    res = analyse(validator, h)
    assert_matches(res, ref, h.ntxn)
    check_witnesses(res, ref)
    bare = analyse(validator, h, witness=False)
    np.testing.assert_array_equal(bare["cls"], ref.cls)
    assert not bare["wit_off"].any() and len(bare["wit_txn"]) == 0 and bare["bfs_levels"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 63, 64, 65, 129])
def test_gpu_fan_batch_boundaries(validator, oracle_mod, k):
    h = fan(k)
    ref = ref_of_history(oracle_mod, h)
    res = analyse(validator, h)
    assert_matches(res, ref, h.ntxn)
    assert res["cls"].tolist() == [GSINGLE | G2] * (k + 1)
    assert res["reach_batches"] == (k + 63) // 64 and res["anti_edges"] == k
    assert res["comp_class"].tolist() == [GSINGLE]
    assert res["wit_off"].tolist() == [0, 2]
    check_witnesses(res, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed3000", "skew1500_0", "skew1500_1"])
def test_gpu_generated_match_reference(validator, oracle_mod, name):
    h = generated(name)
    ref = ref_for(oracle_mod, name, h)
    res = analyse(validator, h)
    gs, gd, gt = validator.dep_graph_edges()
    np.testing.assert_array_equal(gs, ref.s)
    np.testing.assert_array_equal(gd, ref.d)
    np.testing.assert_array_equal(gt, ref.t)
    assert_matches(res, ref, h.ntxn)
    check_witnesses(res, ref)


@pytest.mark.gpu
def test_gpu_larger_case_and_budget(validator, oracle_mod):
    """20000 txns, 15242 of them in cycles, 26355 anti edges: the
    Tarjan-derived bits, the classes that follow from them, every witness;
    and a budget of one batch.  (The reference's G-single bit -- half a
    second here -- is checked as well.)"""
    h = generated("large")
    ref = ref_for(oracle_mod, "large", h)
    res = analyse(validator, h)
    gs, gd, gt = validator.dep_graph_edges()
    np.testing.assert_array_equal(gs, ref.s)
    np.testing.assert_array_equal(gd, ref.d)
    np.testing.assert_array_equal(gt, ref.t)
    print(f"large: txns in cycles {ref.core_nodes} anti edges {ref.anti_edges}; analysis "
          f"{res['ms']:.2f} ms core_nodes {res['core_nodes']} reach_batches {res['reach_batches']} "
          f"sweeps {res['sweeps']} bfs_levels {res['bfs_levels']}")
    np.testing.assert_array_equal(res["cls"] & (G1C | G2), ref.cls & (G1C | G2))
    np.testing.assert_array_equal(res["comp_label"], ref.comp_label)
    has_g1c = ref.comp_class == G1C
    np.testing.assert_array_equal(res["comp_class"][has_g1c], ref.comp_class[has_g1c])
    assert not (res["comp_class"][~has_g1c] == G1C).any()
    assert res["anti_edges"] == res["anti_tested"] == ref.anti_edges == 26355 and ref.core_nodes == 15242
    assert_matches(res, ref, h.ntxn)
    check_witnesses(res, ref)
    part = validator.dep_graph_anomalies(witness=True, max_anti_batches=1)
    assert part["anti_tested"] == 64 < part["anti_edges"] == ref.anti_edges
    assert part["reach_batches"] == 1
    np.testing.assert_array_equal(part["cls"] & (G1C | G2), ref.cls & (G1C | G2))
    assert not ((part["cls"] & GSINGLE) & ~(res["cls"] & GSINGLE)).any()
    # (a closed anti edge among the first 64 <=> the budgeted run found some G-single txn)
    assert bool((part["cls"] & GSINGLE).any()) == bool(np.isin(ref.closed_idx, ref.anti_idx[:64]).any())


@pytest.mark.gpu
def test_gpu_states(oracle_mod):
    v = hsc.Validator(0)
    try:
        v.dep_graph_build(WRITE_SKEW, full=False)
        with pytest.raises(hsc.HscError, match=r"-> -5"):  # HSC_ESTATE
            v.dep_graph_anomalies()
        first = analyse(v, generated("skew1500_0"))
        assert first["comps"][1] > 0
        # a new build: the context's arrays are the new graph's
        res = analyse(v, READ_SKEW)
        ref = ref_of_history(oracle_mod, READ_SKEW)
        assert_matches(res, ref, READ_SKEW.ntxn)
        res = analyse(v, SERIAL)
        assert res["cls"].tolist() == [0, 0, 0] and len(res["comp_label"]) == 0
        assert res["wit_off"].tolist() == [0]
        # the analysis leaves the build as it was
        h = generated("mixed3000")
        ref = ref_for(oracle_mod, "mixed3000", h)
        analyse(v, h)
        scc, st = v.dep_graph_scc_built(h.ntxn)
        np.testing.assert_array_equal(scc, ref.scc)
        gs, gd, gt = v.dep_graph_edges()
        np.testing.assert_array_equal(gs, ref.s)
        np.testing.assert_array_equal(gt, ref.t)
        assert_matches(v.dep_graph_anomalies(), ref, h.ntxn)
    finally:
        v.close()
