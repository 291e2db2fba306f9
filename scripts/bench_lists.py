"""The list-append entry (hsc_dep_graph_resolve_lists) on a
generated history (jepsen.append_history_edn with its injections, txn ids
shuffled), and beside it hsc_dep_graph_resolve on an rw-register history of
config-4 shape in value form cut to the same op count.  After a warm-up call
each, ``--repeats`` calls of each entry: the call's device ms (its uploads
included), min-max; and the build_ms of the graph_build_lists it feeds.

    python scripts/bench_lists.py [--txns 40000] [--keys 600] [--repeats 5]
One JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (HIP initialised by torch first, as in the tests)

from comdb2_amd import hsc  # noqa: E402
from comdb2_amd import jepsen as J  # noqa: E402
from comdb2_amd.workloads import ValueHistory, config4_history, value_history  # noqa: E402


def register_history(nops):
    """config 4 in value form, its first nops ops."""
    v = value_history(config4_history(seed=6, n_txn=max(nops // 5, 16), n_keys=max(nops // 30, 8)))
    n = min(nops, v.nops)
    return ValueHistory(v.txn[:n], v.key[:n], v.is_write[:n], v.value[:n], v.status, v.ntxn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--txns", type=int, default=40000)
    ap.add_argument("--keys", type=int, default=600)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    import lists_model as M
    text, inj = J.append_history_edn(1, n_txns=a.txns, n_keys=a.keys)
    h = M.permuted(J.lhistory_from_append_edn(text).lhistory, 1)
    vh = register_history(h.nops)
    v = hsc.Validator(0)
    try:
        res = v.graph_resolve_lists(h, arrays=False)  # warm-up
        v.graph_build_lists(full=True)
        lists_ms, build_ms = [], []
        for _ in range(a.repeats):
            lists_ms.append(float(v.graph_resolve_lists(h, arrays=False)["ms"]))
            build_ms.append(float(v.graph_build_lists(full=True)["build_ms"]))
        v.dep_graph_resolve(vh, arrays=False)  # warm-up
        reg_ms = [float(v.dep_graph_resolve(vh, arrays=False)["ms"]) for _ in range(a.repeats)]
    finally:
        v.close()
    out = {"txns": int(h.ntxn), "ops": int(h.nops), "appends": int(res["appends"]), "elements": int(res["elements"]),
           "keys": int(res["keys"]), "spine_elements": int(res["spine_elements"]),
           "edge_rows": int(res["ww"] + res["wr"] + res["rw"]), "injected": inj, "repeats": a.repeats,
           "resolve_lists_ms": [round(min(lists_ms), 3), round(max(lists_ms), 3)],
           "build_lists_ms": [round(min(build_ms), 3), round(max(build_ms), 3)],
           "register_ops": int(vh.nops), "register_txns": int(vh.ntxn),
           "resolve_ms": [round(min(reg_ms), 3), round(max(reg_ms), 3)]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
