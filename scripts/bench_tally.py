"""hsc_tally_check and hsc_bank_check: device ms of the call
(upload, sort, passes; min-max of ``--repeats`` calls after a warm-up),
elements per second at the fastest, the host's wall time around the call
(``call_ms``), and beside each -- as context, not as a yardstick: there is no
earlier GPU path and no JVM here -- the time of
``numpy.unique(return_counts=True)`` over the same arrays on one core of the
same box (for bank: of numpy's row sums).

  set_1e6 / set_1e8      adds of distinct values (a third of the elements),
                         97 % acknowledged, a final read that lacks 1 in 1000
                         acknowledged adds and holds every other unacknowledged one
  queue_1e6 / queue_1e8  the same sizes in multiset mode, values drawn from a
                         range an eighth of the enqueues (so they repeat)
  bank_1e6               10^6 reads of 10 accounts, 1 in 1000 skewed

    python scripts/bench_tally.py [--repeats 5] [--big 100000000] [--log profiles/tally_bench.log]
One JSON line per shape, also appended to the log."""
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


def timed(call, repeats):
    """(the reports' device ms, the host's wall ms around each call -- the binding's copies included)"""
    ms, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(float(res["ms"]))
    return ms, wall


def tally_inputs(n, multiset, seed=1):
    rng = np.random.default_rng(seed)
    m = n // 3
    attempt = rng.integers(0, max(m // 8, 1), m) if multiset else rng.permutation(m)
    acked = rng.random(m) < 0.97
    ack = attempt[acked]
    keep = np.where(acked, rng.random(m) >= 0.001, rng.random(m) < 0.5)
    seen = rng.permutation(attempt[keep])
    return attempt.astype(np.int64), ack.astype(np.int64), seen.astype(np.int64)


def measure_tally(v, name, n, multiset, repeats):
    a, k, s = tally_inputs(n, multiset)
    res = v.tally_check(a, k, s, multiset=multiset)  # warm-up
    ms, wall = timed(lambda: v.tally_check(a, k, s, multiset=multiset), repeats)
    t0 = time.perf_counter()
    uniq = [np.unique(x, return_counts=True) for x in (a, k, s)]
    numpy_s = time.perf_counter() - t0
    # the counts numpy gives at once: the totals, and the lost elements in set mode
    assert [res[c] for c in ("attempts", "acks", "seen")] == [len(x) if multiset else len(u) for x, (u, _) in
                                                             zip((a, k, s), uniq)]
    if not multiset:
        assert res["lost"]["count"] == len(np.setdiff1d(uniq[1][0], uniq[2][0], assume_unique=True))
    total = len(a) + len(k) + len(s)
    return {"shape": name, "elements": total, "distinct": int(res["distinct"]), "multiset": multiset,
            "sort_packed": int(res["sort_packed"]), "valid": int(res["valid"]),
            **{c: int(res[c]["count"]) for c in hsc.TALLY_CLASSES}, "repeats": repeats,
            "device_ms": [round(min(ms), 3), round(max(ms), 3)], "elements_per_s": round(total / (min(ms) / 1e3)),
            "call_ms": [round(min(wall), 3), round(max(wall), 3)],
            "numpy_unique_s": round(numpy_s, 3)}


def measure_bank(v, name, n_reads, n, repeats, seed=2):
    rng = np.random.default_rng(seed)
    bal = np.full((n_reads, n), 10, np.int64)
    moved = rng.integers(0, 10, n_reads)
    bal[:, 0] -= moved
    bal[:, 1] += np.where(rng.random(n_reads) < 0.001, 0, moved)  # a skewed read misses the credit
    off = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(n)
    flat = bal.reshape(-1)
    res = v.bank_check(off, flat, n, 10 * n)  # warm-up
    ms, wall = timed(lambda: v.bank_check(off, flat, n, 10 * n), repeats)
    t0 = time.perf_counter()
    bad = int((bal.sum(axis=1) != 10 * n).sum())
    numpy_s = time.perf_counter() - t0
    assert res["bad"] == res["wrong_total"] == bad and res["wrong_n"] == 0
    return {"shape": name, "reads": n_reads, "n": n, "elements": int(flat.size), "bad": bad, "repeats": repeats,
            "device_ms": [round(min(ms), 3), round(max(ms), 3)],
            "elements_per_s": round(flat.size / (min(ms) / 1e3)), "call_ms": [round(min(wall), 3), round(max(wall), 3)],
            "numpy_sum_s": round(numpy_s, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--big", type=int, default=100_000_000, help="elements of the large tally shapes")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "tally_bench.log"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    v = hsc.Validator(0)
    try:
        for job in ((measure_tally, "set_1e6", 1_000_000, False), (measure_tally, "queue_1e6", 1_000_000, True),
                    (measure_bank, "bank_1e6", 1_000_000, 10),
                    (measure_tally, f"set_{a.big:.0e}".replace("+0", ""), a.big, False),
                    (measure_tally, f"queue_{a.big:.0e}".replace("+0", ""), a.big, True)):
            row = job[0](v, *job[1:], a.repeats)
            print(json.dumps(row), flush=True)
            with open(a.log, "a") as f:
                f.write(json.dumps(row) + "\n")
    finally:
        v.close()


if __name__ == "__main__":
    main()
