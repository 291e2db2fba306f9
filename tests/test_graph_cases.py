"""The dependency graph's hand-built cases (tests/graph_cases.py) on the CPU:
the C oracle (oracle/scc_oracle.c) and the independent Python model
(test_graph.py's py_edges / py_scc) agree on every one of them -- inputs the
reference had not seen: arbitrary observed ids, constant key and txn bits,
degenerate layouts -- and every case reaches the branch of graph_build it is
named for, under plan_of's restatement of the host's plan.  The -m gpu file
test_gpu_graph_paths.py then holds the kernels to the same oracle."""
import numpy as np
import pytest

import graph_cases as gc
from test_graph import py_edges, py_scc

NAMES = list(gc.cases())


def check_preconditions(name, case, plan, s, d, t, scc):
    """Every assert names the case and the branch that is no longer reached."""
    h = case.h
    why = f"case {name}: rebuild it (tests/graph_cases.py) --"
    for k, v in case.expect.items():
        assert getattr(plan, k) == v, f"{why} plan.{k} = {getattr(plan, k)!r}, the case needs {v!r}"
    rd = np.asarray(h.is_write) == 0
    obs, txn, key = np.asarray(h.observed, np.int64), np.asarray(h.txn, np.int64), np.asarray(h.key, np.uint64)
    slow = rd & ~plan.compressible
    wtx = txn[~rd]
    for tag in case.tags:
        if tag == "tc":
            assert plan.tc != 0, f"{why} the writers' txns share no constant set bit (pp.tc)"
        elif tag == "kc":
            assert plan.kc != 0, f"{why} the writers' keys share no constant set bit (pp.kc)"
        elif tag in ("slow", "slow_1000"):
            need = 1000 if tag == "slow_1000" else 1
            assert int(slow.sum()) >= need, \
                f"{why} {int(slow.sum())} reads with an incompressible observed id (pk_rw_slow)"
            if tag == "slow_1000":
                assert (obs[slow] < wtx.min()).any() and (obs[slow] > wtx.max()).any(), \
                    f"{why} incompressible observed ids on one side of the writers only"
        elif tag == "ob_self":
            assert (rd & (obs == txn)).any(), f"{why} no read of the txn's own write (ob == r)"
        elif tag == "ob_later":
            assert (rd & (obs > txn)).any(), f"{why} no read observing a later txn (ob > r)"
        elif tag == "ob_last":
            last = {}
            for k, x in zip(key[~rd].tolist(), wtx.tolist()):
                last[k] = max(last.get(k, -1), x)
            assert any(last.get(k, -2) == o for k, o in zip(key[rd].tolist(), obs[rd].tolist())), \
                f"{why} no read of a key's last version"
        elif tag == "key_outside":
            out = rd & ((key & np.uint64(~plan.km & gc.M64)) != np.uint64(plan.kc))
            assert out.any(), f"{why} no read of a key outside the writers' constant bits"
        elif tag == "types7":
            assert int(np.bitwise_or.reduce(t)) == 7, f"{why} the edge types do not OR to ww | wr | rw"
        elif tag == "cycle":
            assert np.bincount(scc, minlength=h.ntxn).max() > 1, f"{why} no component of two txns"
        elif tag == "merged_types":
            assert any(bin(int(x)).count("1") > 1 for x in t), f"{why} no edge of two types"
            ops = np.stack([txn, key.astype(np.int64), rd.astype(np.int64), obs], 1)
            assert len(np.unique(ops[rd], axis=0)) < int(rd.sum()), f"{why} no duplicate read op"
        elif tag in ("bucket_12", "bucket_13"):
            n = int(tag[-2:])
            assert gc.K_PT_E == 12 and (plan.occupancy == n).any(), \
                f"{why} no bucket of exactly {n} writers (kPtE = 12: the bucket line's last entry / overflow)"
        elif tag in ("x_below_base", "x_above_last"):
            c = plan.compressible & (obs >= 0) & ((key & np.uint64(~plan.km & gc.M64)) == np.uint64(plan.kc))
            x = (gc._compress(key[c], plan.km) << np.uint64(plan.tb)) | gc._compress(obs[c].astype(np.uint64), plan.tm)
            ok = (x < plan.pk[0]).any() if tag == "x_below_base" else (x > plan.pk[-1]).any()
            assert ok, f"{why} no compressible read {tag.replace('_', ' ')} of the packed writers"
        elif tag == "all_passes":
            assert not plan.txn_sorted and plan.sort_passes == (plan.B + 7) // 8, \
                f"{why} the ops are in txn order (the sort would skip the txn bits)"
        elif tag == "tile_2048":
            assert plan.km == 0 and plan.nu > 2048, f"{why} one key's run does not cross the unpack's 2048-row tile"
        else:
            raise AssertionError(f"unknown tag {tag}")
    if name.startswith("any_observed[12]") or name == "unsorted":
        occ = plan.occupancy
        assert ((occ > 0) & (occ <= gc.K_PT_E)).any() and (occ > gc.K_PT_E).any(), \
            f"{why} bucket lines and overflowing buckets are not both present"


@pytest.mark.parametrize("name", NAMES)
def test_case_oracle_model_and_branch(oracle_mod, name):
    case = gc.cases()[name]
    h = case.h
    s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
    E = py_edges(h)
    assert sorted(E.items()) == sorted(zip(zip(s.tolist(), d.tolist()), t.tolist()))
    scc = oracle_mod.scc(h.ntxn, s, d)
    np.testing.assert_array_equal(scc, py_scc(h.ntxn, E))
    # (the vectorised raw-row model the large GPU cases are counted with)
    np.testing.assert_array_equal(np.unique(gc.raw_rows(h)), (s.astype(np.uint64) << np.uint64(32)) | d)
    check_preconditions(name, case, gc.plan_of(h), s, d, t, scc)


def test_place_cases_cover_the_block_edges():
    """Writers at the first and last op of the place pass's 4096-op block."""
    for n in gc.PLACE_NOPS:
        h = gc.cases()[f"place[{n}]"].h
        assert len(h.txn) == n and h.is_write[0] and h.is_write[n - 1]
        if n > 4096:
            assert h.is_write[4095] and h.is_write[4096]


def test_big_cut_case_has_more_rows_than_the_fast_cut(oracle_mod):
    """The cut-boundary history: more valid raw rows than kCutFastCap = 65536
    (graph_cut then takes the flag-and-scan path under an all-ones cover)."""
    h = gc.big_cut_history()
    assert gc.plan_of(h).path == "pt"
    assert gc.valid_raw_rows(h) > 65536


def test_ring_case_needs_every_edge(oracle_mod):
    """The op-range cut's rings: each ring's membership hangs on one ww, one
    wr and one rw row -- without any one of them the oracle's components
    change -- and the writers carry constant txn and key bits on the exact
    packed search's path."""
    h, rings = gc.ring_history()
    p = gc.plan_of(h)
    assert p.packs and p.tc != 0 and p.kc != 0 and p.txn_sorted
    s, d, t = oracle_mod.dep_edges(h.txn, h.key, h.is_write, h.observed)
    want = oracle_mod.scc(h.ntxn, s, d)
    sizes = np.bincount(want, minlength=h.ntxn)
    assert (sizes == 3).sum() == len(rings) and sizes.max() == 3  # the chained txns stay apart
    a, b, c = rings[len(rings) // 2]
    for (x, y), bit in (((a, b), 1), ((b, c), 2), ((c, a), 4)):
        i = np.nonzero((s == x) & (d == y))[0]
        assert len(i) == 1 and int(t[i[0]]) == bit  # the ring's only edge of that type
        keep = np.ones(len(s), bool)
        keep[i] = False
        assert not np.array_equal(oracle_mod.scc(h.ntxn, s[keep], d[keep]), want)
    # the ww source writes its key twice (k_cut_txn_ops' dup scan)
    w = (np.asarray(h.txn) == a) & (np.asarray(h.is_write) != 0)
    ks = np.asarray(h.key)[w].tolist()
    assert len(ks) == 3 and ks[0] == ks[2] != ks[1]  # (another write between the two)


@pytest.mark.parametrize("n_nodes,m", [(4096, None), (4097, None), (4096, 24576), (4096, 24577)])
def test_scc_limit_cases_shape(oracle_mod, n_nodes, m):
    """The synthetic cuts of the one-workgroup SCC's limits: the asked node
    and row counts, many 3- and 4-rings, nothing larger."""
    cover, rows, (s, d) = gc.scc_limit_case(n_nodes, m)
    assert int(cover.sum()) == n_nodes and (m is None or len(rows) == m)
    assert len(rows) <= 24576 or m == 24577
    want = oracle_mod.scc(len(cover), s, d)
    sizes = np.bincount(want, minlength=len(cover))
    assert (sizes == 3).sum() > 100 and (sizes == 4).sum() > 100 and sizes.max() == 4
    assert cover[s].all() and cover[d].all()
