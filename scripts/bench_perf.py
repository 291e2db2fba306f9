"""hsc_perf_check: device ms of the call (upload from pageable
host memory, the sorts, the passes, the cells back; min-max of ``--repeats``
calls after a warm-up), its split over the entry's phases (``phase_ms``: rows =
upload + input checks, pair, cells, rate, raw), ops per second at the fastest,
the host's wall time around the call (``call_ms``, the binding's copies
included), and beside it -- as context, not as a yardstick: there is no earlier
GPU path and no JVM here -- the same data sets from numpy on the same box
(stable argsort by process, adjacent rows, lexsort per cell; the per-f work on
a pool of ``--threads`` threads, numpy's sorts releasing the GIL).

  perf_1e7 / perf_1e8   a synthetic history of that many ops: 8 :f values, 64
                        processes each running invoke / completion pairs back
                        to back over 1 h of test time, 2 % :fail, 1 % :info,
                        latencies exponential

    python scripts/bench_perf.py [--repeats 3] [--sizes 10000000 100000000] [--log profiles/perf_bench.log]
One JSON line per shape, also appended to the log."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (HIP initialised by torch first, as in the tests)

from comdb2_amd import hsc  # noqa: E402

NF, NPROC, HOUR = 8, 64, 3600 * 10 ** 9
QS = (0.5, 0.95, 0.99, 1)


def history(n, seed=1):
    """(type, f, process, client, time) in history (time) order."""
    rng = np.random.default_rng(seed)
    m = n // 2  # pairs
    per = m // NPROC
    m = per * NPROC
    gap = HOUR / (2 * per)
    # per process: invoke, completion, invoke, ... at increasing times
    steps = rng.exponential(gap, (NPROC, 2 * per)) + 1
    t = np.cumsum(steps, axis=1).astype(np.int64)
    proc = np.repeat(np.arange(NPROC, dtype=np.uint32), 2 * per)
    f = np.repeat(rng.integers(0, NF, (NPROC, per)).astype(np.uint32), 2, axis=1).reshape(-1)
    u = rng.random((NPROC, per))
    ctype = np.where(u < 0.02, hsc.OP_FAIL, np.where(u < 0.03, hsc.OP_INFO, hsc.OP_OK)).astype(np.uint8)
    typ = np.stack([np.zeros_like(ctype), ctype], axis=2).reshape(-1)
    order = np.argsort(t.reshape(-1), kind="stable")
    return typ[order], f[order], proc[order], np.ones(len(order), np.uint8), t.reshape(-1)[order]


def numpy_perf(typ, f, proc, client, t, threads):
    """The scalars and cells hsc_perf_check gives, through numpy."""
    n = len(typ)
    order = np.argsort(proc, kind="stable")
    st = typ[order]
    same = proc[order][1:] == proc[order][:-1]
    hit = same & (st[:-1] == 0) & (st[1:] != 0)
    inv, comp = order[:-1][hit], order[1:][hit]
    lat = t[comp] - t[inv]
    qb = ((t[inv].astype(np.float64) / 1e9) / 30).astype(np.int64)
    done = np.flatnonzero((typ != 0) & (client != 0))
    rb = ((t[done].astype(np.float64) / 1e9) / 10).astype(np.int64)

    def one_f(k):
        sel = f[inv] == k
        o = np.lexsort((lat[sel], qb[sel]))
        b, l = qb[sel][o], lat[sel][o]
        head = np.flatnonzero(np.r_[True, b[1:] != b[:-1]])
        cnt = np.diff(np.r_[head, len(b)])
        quant = [l[head + np.minimum(cnt - 1, np.floor(cnt * q).astype(np.int64))] for q in QS]
        rs = f[done] == k
        rkey = typ[done][rs].astype(np.int64) << 32 | rb[rs]
        ru, rc = np.unique(rkey, return_counts=True)
        return len(head), cnt, quant, len(ru), rc

    with ThreadPoolExecutor(threads) as ex:
        parts = list(ex.map(one_f, range(NF)))
    return {"paired": int(hit.sum()), "cells": sum(p[0] for p in parts), "rate_cells": sum(p[3] for p in parts),
            "cell_count": np.concatenate([p[1] for p in parts]),
            "cell_lat": np.concatenate([np.stack(p[2], axis=1) for p in parts]),
            "rate_count": np.concatenate([p[4] for p in parts]), "n": n}


def measure(v, name, n, repeats, threads):
    cols = history(n)
    res = v.perf_check(*cols, NF)  # warm-up
    ms, wall, phases = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = v.perf_check(*cols, NF)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(float(res["ms"]))
        phases.append(res["phase_ms"])
    t0 = time.perf_counter()
    want = numpy_perf(*cols, threads)
    numpy_s = time.perf_counter() - t0
    assert (res["paired"], res["cells"], res["rate_cells"]) == (want["paired"], want["cells"], want["rate_cells"])
    assert np.array_equal(res["cell_count"], want["cell_count"]) and np.array_equal(res["cell_lat"], want["cell_lat"])
    assert np.array_equal(res["rate_count"], want["rate_count"])
    best = phases[int(np.argmin(ms))]
    nbytes = sum(a.nbytes for a in cols)
    return {"shape": name, "ops": len(cols[0]), "paired": int(res["paired"]), "cells": int(res["cells"]),
            "rate_cells": int(res["rate_cells"]), "sort_packed": int(res["sort_packed"]), "repeats": repeats,
            "device_ms": [round(min(ms), 3), round(max(ms), 3)], "ops_per_s": round(len(cols[0]) / (min(ms) / 1e3)),
            "phase_ms": {k: round(float(x), 3) for k, x in best.items()}, "upload_mb": round(nbytes / 1e6, 1),
            "call_ms": [round(min(wall), 3), round(max(wall), 3)], "numpy_s": round(numpy_s, 3),
            "numpy_threads": threads}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000_000, 100_000_000])
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "perf_bench.log"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    v = hsc.Validator(0)
    try:
        for n in a.sizes:
            row = measure(v, f"perf_{n:.0e}".replace("+0", ""), n, a.repeats, a.threads)
            print(json.dumps(row), flush=True)
            with open(a.log, "a") as f:
                f.write(json.dumps(row) + "\n")
    finally:
        v.close()


if __name__ == "__main__":
    main()
