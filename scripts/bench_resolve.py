"""Version resolution (hsc_dep_graph_resolve) on histories of
config-4 shape in value form, with 1 % aborted and 0.1 % unknown txns.  Per
size, after a warm-up call each, three repeats of: the resolve call's device
ms (its uploads included), the build_ms of the dep_graph_build_resolved it
feeds, and the build_ms of a plain dep_graph_build of the equivalent committed
history in the same run; and once the numpy time of the same resolution on one
core (lexsort + searchsorted).  The numpy resolution also yields the committed
history, whose counts must equal the GPU's.

    python scripts/bench_resolve.py [--sizes 1000000,16700000] [--repeats 3] [--resolve-only] [--no-numpy]
--resolve-only: the resolve calls alone (for a kernel trace).  One JSON line per size."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (HIP initialised by torch first, as in the tests)

from comdb2_amd import hsc  # noqa: E402
from comdb2_amd.workloads import History, config4_history, value_history  # noqa: E402

OK, ABORTED, UNKNOWN = 0, 1, 2
INIT = np.uint64(0xFFFFFFFFFFFFFFFF)


def numpy_resolve(v):
    """(obs_txn per op (-1 initial / write, -2 none), seconds of the sort and the search)."""
    t0 = time.perf_counter()
    w = np.nonzero(v.is_write)[0]
    o = np.lexsort((v.value[w], v.key[w]))
    wk, wv, wt = v.key[w][o], v.value[w][o], v.txn[w][o]
    comp = (wk << np.uint64(32)) | wv  # config-4 shape: keys and values below 2^32
    r = np.nonzero((v.is_write == 0) & (v.value != INIT))[0]
    q = (v.key[r] << np.uint64(32)) | v.value[r]
    at = np.searchsorted(comp, q)
    hit = comp[np.minimum(at, len(comp) - 1)] == q
    obs = np.full(v.nops, -1, np.int64)
    obs[r] = np.where(hit, wt[np.minimum(at, len(comp) - 1)].astype(np.int64), -2)
    return obs, time.perf_counter() - t0


def committed_history(v, obs):
    """The lowering of §5g in numpy (every write of these histories is final)."""
    st = v.status
    in_c = st == OK
    rd = np.nonzero(obs >= 0)[0]
    rd = rd[(obs[rd] != v.txn[rd]) & (st[obs[rd]] == UNKNOWN)]
    while True:
        new = rd[in_c[v.txn[rd]] & ~in_c[obs[rd]]]
        if not len(new):
            break
        in_c[obs[new]] = True
    cid = np.cumsum(in_c) - 1
    aborted_read = (obs >= 0) & (st[np.maximum(obs, 0)] == ABORTED) & (obs != v.txn)
    keep = in_c[v.txn] & ~aborted_read & (obs != -2)
    o = obs[keep]
    low = History(cid[v.txn[keep]].astype(np.uint32), v.key[keep], v.is_write[keep],
                  np.where(o >= 0, cid[np.maximum(o, 0)], -1).astype(np.int64), int(in_c.sum()))
    return low, int((aborted_read & in_c[v.txn]).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,16700000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--resolve-only", action="store_true", help="the resolve calls alone (for a kernel trace)")
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    val = hsc.Validator(0)
    for n_txn in [int(x) for x in a.sizes.split(",")]:
        h = config4_history(n_txn=n_txn, n_keys=max(1000, n_txn // 10))
        rng = np.random.default_rng(n_txn)
        status = rng.choice([OK, ABORTED, UNKNOWN], size=n_txn, p=[0.989, 0.01, 0.001]).astype(np.uint8)
        v = value_history(h, status)
        out = dict(ntxn=n_txn, nops=v.nops)
        val.dep_graph_resolve(v, arrays=False)  # warm (buffers)
        runs = [val.dep_graph_resolve(v, arrays=False) for _ in range(a.repeats)]
        r = runs[-1]
        out["resolve_ms"] = [round(x["ms"], 3) for x in runs]
        out.update({k: r[k] for k in ("writes", "reads", "kept_ops", "ncommitted", "recovered", "aborted", "dropped",
                                      "g1a_reads", "g1b_reads", "sweeps", "sort_path")})
        if not a.resolve_only:
            val.dep_graph_build_resolved(full=True)
            b = [val.dep_graph_build_resolved(full=True) for _ in range(a.repeats)]
            out["build_resolved_ms"] = [round(x["build_ms"], 3) for x in b]
            out["edges"] = b[-1]["edges"]
            if not a.no_numpy:
                obs, secs = numpy_resolve(v)
                out["numpy_resolve_s"] = round(secs, 3)
                low, g1a = committed_history(v, obs)
                assert (low.nops, low.ntxn, g1a) == (r["kept_ops"], r["ncommitted"], r["g1a_reads"]), \
                    (low.nops, low.ntxn, g1a)
                val.dep_graph_build(low, full=True)
                p = [val.dep_graph_build(low, full=True) for _ in range(a.repeats)]
                out["plain_build_ms"] = [round(x["build_ms"], 3) for x in p]
                assert p[-1]["edges"] == out["edges"], (p[-1]["edges"], out["edges"])
        print(json.dumps(out), flush=True)
    val.close()


if __name__ == "__main__":
    main()
