"""hsc_linear_check on three shapes, device ms of the call
(upload and launch; min-max of ``--repeats`` calls after a warm-up), events per
second at the fastest, the peak configurations of a step, and beside each the
time of the Python model (tests/linear_model.py) on one core of the same box:

  one_key    one key of 10 000 ops at 10 processes: one workgroup on one CU
  many_keys  1024 keys of 1000 ops at 5 processes with :info ops (32 generated
             histories, each used for 32 keys; the model runs the 32 and its
             time is multiplied)
  near_cap   one key, 9 open writes of distinct values under a stream of nil
             reads: every step holds 9 * 2^8 + 1 = 2305 configurations

    python scripts/bench_linear.py [--repeats 5] [--log profiles/linear_bench.log]
One JSON line per shape, also appended to the log."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (HIP initialised by torch first, as in the tests)

import linear_model as LM  # noqa: E402
from comdb2_amd import hsc  # noqa: E402
from comdb2_amd import jepsen as J  # noqa: E402


def one_key():
    text, _ = J.cas_register_history_edn(11, n_ops=10000, n_procs=10, info=0.0)
    return J.lin_ops_from_register_edn(text).arrays(), 1


def many_keys(distinct=32, copies=32):
    parts = []
    for seed in range(distinct):
        text, _ = J.cas_register_history_edn(100 + seed, n_ops=1000, n_procs=5, info=0.02, max_open=4)
        o = J.lin_ops_from_register_edn(text)
        parts.append({k: getattr(o, k).tolist() for k in ("f", "a", "b", "invoke", "complete")})
    return LM.columns(parts * copies), LM.columns(parts), copies


def near_cap(reads=200):
    k = 9
    f = [LM.WRITE] * k + [LM.READ] * reads
    a = list(range(1, k + 1)) + [LM.NIL] * reads
    invoke = list(range(k)) + [k + 2 * j for j in range(reads)]
    complete = [LM.RT_OPEN] * k + [k + 2 * j + 1 for j in range(reads)]
    return LM.columns([dict(f=f, a=a, b=[LM.NIL] * len(f), invoke=invoke, complete=complete)]), 1


def measure(v, name, ops, model_ops, scale, repeats):
    res = v.linear_check(ops)  # warm-up
    ms = [float(v.linear_check(ops)["ms"]) for _ in range(repeats)]
    t0 = time.perf_counter()
    ref = LM.check(model_ops)
    model_s = (time.perf_counter() - t0) * scale
    assert ref["bad"] * scale == res["bad"] and ref["unknown"] * scale == res["unknown"]
    assert ref["expanded"] * scale == res["expanded"]
    return {"shape": name, "keys": int(ops["nkeys"]), "ops": int(len(ops["key"])), "events": int(res["events"]),
            "bad": int(res["bad"]), "unknown": int(res["unknown"]), "expanded": int(res["expanded"]),
            "peak_configs": int(np.max(res["peak_configs"])), "repeats": repeats,
            "device_ms": [round(min(ms), 3), round(max(ms), 3)],
            "events_per_s": round(res["events"] / (min(ms) / 1e3)), "model_s": round(model_s, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "linear_bench.log"))
    a = ap.parse_args()
    ops1, _ = one_key()
    opsm, opsm_model, copies = many_keys()
    opsc, _ = near_cap()
    v = hsc.Validator(0)
    try:
        rows = [measure(v, "one_key", ops1, ops1, 1, a.repeats),
                measure(v, "many_keys", opsm, opsm_model, copies, a.repeats),
                measure(v, "near_cap", opsc, opsc, 1, a.repeats)]
    finally:
        v.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
