"""The real-time order as dependency edges (hsc_dep_graph_stage_realtime,
DESIGN.md §5e) on histories of config-4 shape: txn ids are commit order, txn
t belongs to process t % P and completes at 2 t + 1, invoked a random span
before that and after its process's previous completion -- P txns open at
once.  Per size and P: the staged edge count, the staging call's device time
(sort + suffix minima + count + scan + emit) and wall time, build_ms / scc_ms
of the same history with and without the real-time edges, and a vectorised
numpy restatement of the same interval computation (argsort, minimum.accumulate
on the reversed array, two searchsorted) on one core, checked to give the same
number of edges (and, at the smaller size, the same edges).

    python scripts/bench_realtime.py [--sizes 1000000,16700000] [--procs 8,64] [--stage-only]
One JSON line per (size, P)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (HIP initialised by torch first, as in the tests)

from comdb2_amd import hsc  # noqa: E402
from comdb2_amd.workloads import History, config4_history  # noqa: E402


def intervals(n, procs, seed=0):
    rng = np.random.default_rng(seed)
    cpl = 2 * np.arange(n, dtype=np.int64) + 1
    inv = np.maximum(cpl - rng.integers(0, 2 * procs, size=n), 0)
    return inv.astype(np.uint64), cpl.astype(np.uint64)


def numpy_reduction(inv, cpl):
    """(edge count, src, p, q, order) by the kernels' own formula."""
    order = np.argsort(inv, kind="stable")
    si, sc = inv[order], cpl[order]
    suf = np.minimum.accumulate(sc[::-1])[::-1]
    closed = np.nonzero(cpl != np.uint64(hsc.RT_OPEN))[0]
    p = np.searchsorted(si, cpl[closed], side="right")
    has = p < len(inv)
    closed, p = closed[has], p[has]
    q = np.searchsorted(si, suf[p], side="right")
    return int((q - p).sum()), closed, p, q, order


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,16700000")
    ap.add_argument("--procs", default="8,64")
    ap.add_argument("--stage-only", action="store_true", help="no history, no builds (for a kernel trace)")
    ap.add_argument("--check-edges-below", type=int, default=2_000_000)
    a = ap.parse_args()
    v = hsc.Validator(0)
    for n in [int(x) for x in a.sizes.split(",")]:
        h = None
        plain = {}
        if not a.stage_only:
            h = config4_history(n_txn=n, n_keys=max(1, n // 10))
            v.dep_graph_build(h, full=True)  # warm (buffers)
            plain = v.dep_graph_build(h, full=True)
            _, st = v.dep_graph_scc_built(n)
            plain["scc_ms"], plain["cycles"] = st["scc_ms"], st["nontrivial_sccs"]
        for procs in [int(x) for x in a.procs.split(",")]:
            inv, cpl = intervals(n, procs)
            t0 = time.perf_counter()
            want, src, p, q, order = numpy_reduction(inv, cpl)
            cpu_s = time.perf_counter() - t0
            v.dep_graph_stage_realtime(inv, cpl)  # warm (buffers)
            t0 = time.perf_counter()
            st = v.dep_graph_stage_realtime(inv, cpl)
            wall_s = time.perf_counter() - t0
            out = dict(ntxn=n, procs=procs, rt_edges=st["edges"], stage_ms=round(st["ms"], 3),
                       stage_wall_ms=round(1e3 * wall_s, 3), numpy_1core_ms=round(1e3 * cpu_s, 1),
                       numpy_edges=want, equal=st["edges"] == want)
            empty = History(np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint8),
                            np.zeros(0, np.int64), n)
            if n < a.check_edges_below:  # the edges themselves, through a build of no ops
                v.dep_graph_build(empty, full=True)
                s, d, t = v.dep_graph_edges()
                cnt = q - p
                pos = np.repeat(p, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
                rows = np.sort((np.repeat(src, cnt).astype(np.uint64) << np.uint64(32)) | order[pos].astype(np.uint64))
                got = (s.astype(np.uint64) << np.uint64(32)) | d.astype(np.uint64)
                out["equal"] = bool(out["equal"] and np.array_equal(got, rows) and (t == 8).all())
            else:  # leave nothing staged
                v.dep_graph_build(empty, full=False)
            if h is not None:
                for _ in range(2):  # (the first build grows the edge buffers)
                    v.dep_graph_stage_realtime(inv, cpl)
                    b = v.dep_graph_build(h, full=True)
                _, sst = v.dep_graph_scc_built(n)
                out.update(build_ms=round(plain["build_ms"], 3), scc_ms=round(plain["scc_ms"], 3),
                           edges=plain["edges"], cycles=plain["cycles"],
                           build_ms_rt=round(b["build_ms"], 3), scc_ms_rt=round(sst["scc_ms"], 3),
                           edges_rt=b["edges"], cycles_rt=sst["nontrivial_sccs"])
            print(json.dumps(out), flush=True)
    v.close()


if __name__ == "__main__":
    main()
