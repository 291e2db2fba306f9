"""hsc_linear_check_wide (the wide tier) on the keys the LDS
tier leaves unknown: device ms (min-max of ``--repeats`` calls after a
warm-up; ``wide_ms`` is the wide rounds, ``ms`` the whole call) and expansions
per second at the fastest:

  reference  64 keys of the reference's shape past the LDS caps: 200 ops at 5
             processes, a fifth of the writes and cas ``:info``, at most 9, 10,
             11 or 12 of them per key (16 seeds each), max_configs 2^17
  one_step   one key, 20 concurrent writes of one value under a read: 2^20
             configurations in one step, at the default limits
  lds_only   the first shape through hsc_linear_check: what it leaves unknown

    python scripts/bench_linear_wide.py [--repeats 5] [--log profiles/linear_wide_bench.log]
One JSON line per shape, also appended to the log."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (HIP initialised by torch first, as in the tests)

import linear_model as LM  # noqa: E402
from comdb2_amd import hsc  # noqa: E402
from comdb2_amd import jepsen as J  # noqa: E402


def reference(seeds=16, opens=(9, 10, 11, 12)):
    parts = []
    for max_open in opens:
        for seed in range(1, seeds + 1):
            text, _ = J.cas_register_history_edn(seed, n_ops=200, n_procs=5, info=0.2, max_open=max_open)
            o = J.lin_ops_from_register_edn(text)
            parts.append({k: getattr(o, k).tolist() for k in ("f", "a", "b", "invoke", "complete")})
    return LM.columns(parts)


def one_step(k=20):
    return LM.columns([LM.concurrent_writes(k, values=[7] * k)])


def row(name, ops, res, ms, repeats):
    return {"shape": name, "keys": int(ops["nkeys"]), "ops": int(len(ops["key"])), "events": int(res["events"]),
            "bad": int(res["bad"]), "unknown": int(res["unknown"]), "expanded": int(res["expanded"]),
            "peak_configs": int(np.max(res["peak_configs"])), "repeats": repeats,
            "device_ms": [round(min(ms), 3), round(max(ms), 3)]}


def measure_wide(v, name, ops, repeats, **limits):
    res = v.linear_check_wide(ops, **limits)  # warm-up
    runs = [v.linear_check_wide(ops, **limits) for _ in range(repeats)]
    assert all(r["expanded"] == res["expanded"] and r["unknown"] == res["unknown"] for r in runs)
    wide = [float(r["wide_ms"]) for r in runs]
    causes = np.bincount(res["cause"][res["verdict"] == hsc.LIN_UNKNOWN], minlength=5).tolist()
    out = row(name, ops, res, [float(r["ms"]) for r in runs], repeats)
    out.update({"wide_ms": [round(min(wide), 3), round(max(wide), 3)], "escalated": int(res["escalated"]),
                "resolved": int(res["resolved"]), "rounds": int(res["rounds"]),
                "unknown_causes": dict(zip(("none", "slots", "configs", "budget", "states"), causes)),
                "wide_expanded": int(res["wide_expanded"]), "table_bytes": int(res["table_bytes"]),
                "expansions_per_s": round(res["wide_expanded"] / (min(wide) / 1e3)) if min(wide) > 0 else None})
    return out


def measure_lds(v, name, ops, repeats):
    res = v.linear_check(ops)  # warm-up
    ms = [float(v.linear_check(ops)["ms"]) for _ in range(repeats)]
    return row(name, ops, res, ms, repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "linear_wide_bench.log"))
    a = ap.parse_args()
    ref, one = reference(), one_step()
    v = hsc.Validator(0)
    try:
        rows = [measure_wide(v, "reference", ref, a.repeats, max_configs=1 << 17),
                measure_wide(v, "one_step", one, a.repeats),
                measure_lds(v, "lds_only", ref, a.repeats)]
    finally:
        v.close()
    assert rows[1]["peak_configs"] == 1 << 20 and rows[1]["expanded"] == (1 << 21) - 2 and rows[1]["unknown"] == 0
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    with open(a.log, "a") as f:
        for r in rows:
            print(json.dumps(r))
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
