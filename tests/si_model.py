"""CPU reference of hsc_dep_graph_si (include/hip_serial.h):
which cycles of a typed dependency graph have no two adjacent anti edges.

* E1 = edges with type & 11 (ww, wr or rt bit); an anti edge has type == 4
  exactly; only edges whose ends share a component (oracle Tarjan) matter.
* Product graph P: txn v becomes 2v ("reached by an E1 edge") and 2v + 1
  ("reached by an anti edge"); an E1 edge u -> v gives 2u -> 2v and
  2u + 1 -> 2v, an anti edge 2u -> 2v + 1 only.
* nonadj[v] = 2v or 2v + 1 lies in a component of P with >= 2 nodes.

ref_si builds P with numpy and runs the oracle's Tarjan on it.  For tiny graphs
the statement is also read literally (every simple cycle enumerated), and the
closed-walk -> simple-cycle reduction of the header is restated in plain
Python."""
from collections import deque

import numpy as np

E1_MASK, ANTI = 11, 4


class SiRef:
    """nonadj[ntxn], comp_label / comp_nonadj, comps / txns, core_nodes,
    product_edges, and the edges (s, d, t), scc, inside."""


def ref_si(oracle_mod, ntxn, s, d, t):
    r = SiRef()
    s, d, t = (np.asarray(x, np.int64) for x in (s, d, t))
    r.s, r.d, r.t = s, d, t
    scc = oracle_mod.scc(ntxn, s, d).astype(np.int64) if ntxn else np.zeros(0, np.int64)
    r.scc = scc
    nontriv = np.bincount(scc, minlength=ntxn)[scc] > 1 if ntxn else np.zeros(0, bool)
    inside = (scc[s] == scc[d]) & (s != d)
    r.inside = inside
    e1 = inside & ((t & E1_MASK) != 0)
    anti = inside & (t == ANTI)
    assert (e1 | anti).sum() == inside.sum() and not (e1 & anti).any()
    ps = np.concatenate([2 * s[e1], 2 * s[e1] + 1, 2 * s[anti]])
    pd = np.concatenate([2 * d[e1], 2 * d[e1], 2 * d[anti] + 1])
    order = np.lexsort((pd, ps))  # the oracle's Tarjan wants rows sorted by (src, dst)
    ps, pd = ps[order], pd[order]
    r.ps, r.pd = ps, pd
    pscc = oracle_mod.scc(2 * ntxn, ps, pd).astype(np.int64) if ntxn else np.zeros(0, np.int64)
    r.pscc = pscc
    big = np.bincount(pscc, minlength=2 * ntxn)[pscc] > 1 if ntxn else np.zeros(0, bool)
    r.nonadj = (big[0::2] | big[1::2]).astype(np.uint8)
    r.comp_label = np.unique(scc[nontriv]).astype(np.uint32) if ntxn else np.zeros(0, np.uint32)
    flag = np.zeros(ntxn, bool)
    if ntxn:
        flag[scc[r.nonadj != 0]] = True
    r.comp_nonadj = flag[r.comp_label.astype(np.int64)].astype(np.uint8)
    r.comps = int(r.comp_nonadj.sum())
    r.txns = int(r.nonadj.sum())
    r.core_nodes = int(nontriv.sum())
    r.core_edges = int(inside.sum())
    r.product_edges = int(inside.sum() + e1.sum())
    return r


def ref_of_history(oracle_mod, h):
    s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
    return ref_si(oracle_mod, h.ntxn, s, d, t)


# ---------------------------------------------------------------------------
# the literal statement (tiny graphs)
# ---------------------------------------------------------------------------
def good_cycle(types):
    """No two cyclically consecutive anti edges."""
    n = len(types)
    return not any(types[i] == ANTI and types[(i + 1) % n] == ANTI for i in range(n))


def simple_cycles(n, edges):
    """Every simple cycle of >= 2 nodes as a node list starting at its
    smallest node.  edges: {(u, v): type}."""
    adj = {}
    for (u, v) in edges:
        if u != v:
            adj.setdefault(u, []).append(v)
    out = []

    def walk(start, path, on):
        for w in adj.get(path[-1], ()):
            if w == start:
                if len(path) >= 2:
                    out.append(list(path))
            elif w > start and w not in on:
                on.add(w)
                path.append(w)
                walk(start, path, on)
                path.pop()
                on.discard(w)

    for v in range(n):
        walk(v, [v], {v})
    return out


def literal_good_nodes(n, edges):
    """Txns on some simple cycle without two adjacent anti edges."""
    hit = set()
    for cyc in simple_cycles(n, edges):
        ty = [edges[(cyc[i], cyc[(i + 1) % len(cyc)])] for i in range(len(cyc))]
        if good_cycle(ty):
            hit.update(cyc)
    return hit


# ---------------------------------------------------------------------------
# closed walk -> simple cycle
# ---------------------------------------------------------------------------
def reduce_walk(txns, types):
    """types[i]: the edge txns[i] -> txns[i + 1] (cyclically).  Split at the
    first repeated txn into the two closed halves; a half inherits every
    adjacency but the one at the split.  Keep a half without adjacent anti
    edges there, the shorter if both are good; repeat until simple."""
    txns, types = list(txns), list(types)
    while True:
        seen, i, j = {}, None, None
        for k, v in enumerate(txns):
            if v in seen:
                i, j = seen[v], k
                break
            seen[v] = k
        if j is None:
            return txns, types
        n = len(txns)
        in_ok = not (types[j - 1] == ANTI and types[i] == ANTI)
        out_ok = not (types[(i - 1) % n] == ANTI and types[j] == ANTI)
        assert in_ok or out_ok
        if in_ok and (not out_ok or j - i <= n - (j - i)):
            txns, types = txns[i:j], types[i:j]
        else:
            txns, types = txns[:i] + txns[j:], types[:i] + types[j:]
        assert len(txns) >= 2


def product_walk(edges, a, b):
    """A closed walk through the edge a -> b without two cyclically
    consecutive anti edges, found as the device finds it: a BFS over P from
    a lift's head back to its tail.  None when no lift of a -> b lies on a
    closed walk of P."""
    adj = {}
    for (u, v), ty in edges.items():
        if u == v:
            continue
        if ty & E1_MASK:
            adj.setdefault(2 * u, []).append(2 * v)
            adj.setdefault(2 * u + 1, []).append(2 * v)
        else:
            adj.setdefault(2 * u, []).append(2 * v + 1)
    ty = edges[(a, b)]
    anti = not (ty & E1_MASK)
    head = 2 * b + (1 if anti else 0)
    for tail in ([2 * a] if anti else [2 * a, 2 * a + 1]):
        par = {head: None}
        todo = deque([head])
        while todo and tail not in par:
            x = todo.popleft()
            for w in adj.get(x, ()):
                if w not in par:
                    par[w] = x
                    todo.append(w)
        if tail not in par:
            continue
        nodes = [tail]
        while nodes[-1] != head:
            nodes.append(par[nodes[-1]])
        nodes.reverse()  # head .. tail
        txns = [x >> 1 for x in nodes]
        types = [edges[(txns[k], txns[k + 1])] for k in range(len(txns) - 1)] + [ty]
        return txns, types
    return None


def check_si_witnesses(res, scc, s, d, t):
    """Every property the header promises of a witness: nonempty exactly for
    the flagged components, simple, inside the component, every step an edge
    with its type bits, no two cyclically consecutive anti edges."""
    edge = {(int(a), int(b)): int(c) for a, b, c in zip(s.tolist(), d.tolist(), t.tolist())}
    off = res["wit_off"]
    assert len(off) == len(res["comp_label"]) + 1 and off[0] == 0
    assert off[-1] == len(res["wit_txn"]) == len(res["wit_type"])
    for c, (lab, f) in enumerate(zip(res["comp_label"].tolist(), res["comp_nonadj"].tolist())):
        tx = res["wit_txn"][off[c]:off[c + 1]].tolist()
        ty = res["wit_type"][off[c]:off[c + 1]].tolist()
        if not f:
            assert tx == []
            continue
        assert len(tx) >= 2 and len(set(tx)) == len(tx)
        assert all(scc[v] == lab for v in tx)
        for i, v in enumerate(tx):
            assert edge.get((v, tx[(i + 1) % len(tx)])) == ty[i], "witness step is not an edge of the build"
        assert good_cycle(ty)
