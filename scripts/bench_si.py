"""Snapshot isolation from the dependency graph (hsc_dep_graph_si, DESIGN.md
§5f) beside the anomaly analysis of §5d on the same two graphs: the larger
case of tests/test_anomaly.py and STRESS[1] of tests/test_graph.py (giant
components).  Per graph, after a warm-up call each, three repeats of
dep_graph_anomalies(), dep_graph_anomalies(max_anti_batches=16) and
dep_graph_si(): device ms of each call (its graph_scc runs included), and for
the new analysis the product graph's nodes and edges, the SCC rounds and
iterations of its two runs and the witness search's BFS levels.

    python scripts/bench_si.py [--graphs large,stress1] [--repeats 3] [--si-only]
One JSON line per graph."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (HIP initialised by torch first, as in the tests)

from comdb2_amd import hsc  # noqa: E402
from comdb2_amd.workloads import config4_history  # noqa: E402


def graph(name):
    if name == "large":
        from test_anomaly import generated
        return generated("large")
    if name == "stress1":
        from test_graph import STRESS
        return config4_history(**STRESS[1])
    raise KeyError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="large,stress1")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--si-only", action="store_true", help="the new analysis alone (for a kernel trace)")
    a = ap.parse_args()
    v = hsc.Validator(0)
    for name in a.graphs.split(","):
        h = graph(name)
        st = v.dep_graph_build(h, full=True)
        _, sst = v.dep_graph_scc_built(h.ntxn)
        out = dict(graph=name, ntxn=h.ntxn, edges=st["edges"], scc_ms=round(sst["scc_ms"], 3),
                   components=sst["nontrivial_sccs"])
        calls = [("si_ms", lambda: v.dep_graph_si())]
        if not a.si_only:
            calls = [("anomalies_ms", lambda: v.dep_graph_anomalies()),
                     ("anomalies_16_ms", lambda: v.dep_graph_anomalies(max_anti_batches=16))] + calls
        for key, call in calls:
            call()  # warm (buffers)
            runs = [call() for _ in range(a.repeats)]
            out[key] = [round(r["ms"], 3) for r in runs]
            r = runs[-1]
            if key == "si_ms":
                out.update(core_nodes=r["core_nodes"], product_nodes=r["product_nodes"],
                           product_edges=r["product_edges"], si_scc_rounds=r["scc_rounds"],
                           si_scc_iterations=r["scc_iterations"], si_bfs_levels=r["bfs_levels"],
                           si_comps=r["comps"], si_txns=r["txns"],
                           si_no_witness_ms=round(v.dep_graph_si(witness=False)["ms"], 3))
            else:
                out[key.replace("_ms", "_sweeps")] = r["sweeps"]
                out[key.replace("_ms", "_bfs_levels")] = r["bfs_levels"]
                out["anti_edges"] = r["anti_edges"]
        print(json.dumps(out), flush=True)
    v.close()


if __name__ == "__main__":
    main()
