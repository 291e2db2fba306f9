"""hsc_counter_check / hsc_queue_check: device ms of the call
(upload from pageable host memory, the sorts, the scans, the reports back;
min-max of ``--repeats`` calls after a warm-up), rows per second at the fastest,
the host's wall time around the call (``call_ms``, the binding's copies and the
entry's host-side row check included) and beside it -- as context, not as a
yardstick: there is no earlier GPU path and no JVM here -- the same report from
the numpy formulation of tests/count_model.py on the same box, which the script
asserts the GPU's equals field by field (rows above ``--numpy-max`` skip it).

  counter_<n>_k<keys>   n rows: batches of 64 processes, each invoking then
                        completing one op (half adds of 1 .. 5, half reads at
                        their lower bound; 2 % :fail, 1 % :info), keys uniform
  queue_<n>_k<keys>     n rows, 60 % enqueues, a dequeue taking its key's
                        enqueue of the same rank; both models, final queues on

    python scripts/bench_count.py [--repeats 3] [--sizes 1000000 100000000] [--keys 1 100000]
                                  [--log profiles/count_bench.log]
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

import count_model as CM  # noqa: E402
from comdb2_amd import hsc  # noqa: E402

NPROC = 64


def counter_history(n, nkeys, seed=1):
    """(type, f, process, value, key): batch b is 64 invokes, then their 64
    completions; an :info completion retires its process id."""
    rng = np.random.default_rng(seed)
    nb = max(n // (2 * NPROC), 1)
    m = nb * NPROC
    u = rng.random((nb, NPROC))
    comp = np.where(u < 0.02, hsc.OP_FAIL, np.where(u < 0.03, hsc.OP_INFO, hsc.OP_OK)).astype(np.uint8)
    info = comp == hsc.OP_INFO
    proc = (np.arange(NPROC)[None, :] + NPROC * (np.cumsum(info, axis=0) - info)).astype(np.uint32)
    f = rng.integers(0, 2, (nb, NPROC)).astype(np.uint8)
    val = rng.integers(1, 6, (nb, NPROC)).astype(np.int64)
    key = rng.integers(0, nkeys, (nb, NPROC)).astype(np.uint32)
    two = lambda a, b: np.stack([a, b], axis=1).reshape(-1)  # noqa: E731
    typ = two(np.zeros_like(comp), comp)
    # (an ok read's value is a placeholder until measure_counter places it; a failed read keeps its nil)
    value = two(np.where(f == hsc.CNT_READ, hsc.CNT_NIL, val),
                np.where(f == hsc.CNT_READ, np.where(comp == hsc.OP_OK, 0, hsc.CNT_NIL), val))
    assert len(typ) == 2 * m
    return typ, two(f, f), two(proc, proc), value, two(key, key)


def timed(call, repeats):
    res = call()  # warm-up
    ms, wall = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(float(res["ms"]))
    return res, ms, wall


def row_of(name, n, nkeys, res, ms, wall, nbytes, numpy_s, extra):
    row = {"shape": name, "rows": n, "keys": nkeys, "sort_packed": int(res["sort_packed"]),
           "device_ms": [round(min(ms), 3), round(max(ms), 3)], "rows_per_s": round(n / (min(ms) / 1e3)),
           "upload_mb": round(nbytes / 1e6, 1), "call_ms": [round(min(wall), 3), round(max(wall), 3)],
           "numpy_s": None if numpy_s is None else round(numpy_s, 3)}
    row.update(extra)
    return row


def measure_counter(v, n, nkeys, repeats, with_numpy):
    t, f, p, val, key = counter_history(n, nkeys)
    n = len(t)
    k = None if nkeys == 1 else key
    numpy_s = None
    # the reads take their lower bound (no read value moves a bound)
    if with_numpy:
        t0 = time.perf_counter()
        want = CM.counter_np(t, f, p, val, key, nkeys)
        numpy_s = time.perf_counter() - t0
        lower, rop = want["lower"], want["read_op"]
    else:
        first = v.counter_check(t, f, p, val, k, nkeys)
        lower, rop = first["lower"], first["read_op"]
    val = val.copy()
    val[rop] = lower
    res, ms, wall = timed(lambda: v.counter_check(t, f, p, val, k, nkeys), repeats)
    assert res["bad_reads"] == 0 and res["unknown"] == 0 and res["reads"] == len(rop)
    if with_numpy:
        want["value"] = lower
        want["bad_reads"] = want["n_listed"] = want["bad"] = 0
        want["errors"][:] = 0
        want["verdict"][:] = 0
        want["listed_read"] = want["listed_read"][:0]
        CM.assert_same(res, want, CM.COUNTER_FIELDS, CM.COUNTER_SCALARS)
    nbytes = sum(a.nbytes for a in (t, f, p, val)) + (0 if k is None else key.nbytes)
    return row_of(f"counter_{n:.0e}_k{nkeys}".replace("+0", ""), n, nkeys, res, ms, wall, nbytes, numpy_s,
                  {"reads": int(res["reads"])})


def measure_queue(v, n, nkeys, fifo, repeats, with_numpy):
    f, val, key = CM.gen_queue(2, n, nkeys, nvalues=1 << 20)
    k = None if nkeys == 1 else key
    res, ms, wall = timed(lambda: v.queue_check(f, val, k, nkeys, fifo=fifo, final=True), repeats)
    numpy_s = None
    if with_numpy:
        t0 = time.perf_counter()
        want = CM.queue_np(f, val, key, nkeys, fifo=fifo, final=True)
        numpy_s = time.perf_counter() - t0
        CM.assert_same(res, want, CM.QUEUE_FIELDS, CM.QUEUE_SCALARS)
    nbytes = f.nbytes + val.nbytes + (0 if k is None else key.nbytes)
    name = f"queue_{'fifo' if fifo else 'unordered'}_{n:.0e}_k{nkeys}".replace("+0", "")
    return row_of(name, n, nkeys, res, ms, wall, nbytes, numpy_s,
                  {"bad_keys": int(res["bad"]), "final": int(res["n_final"])})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 100_000_000])
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 100_000])
    ap.add_argument("--numpy-max", type=int, default=1 << 62, help="rows above this skip the numpy comparison")
    ap.add_argument("--only", choices=["counter", "queue"], default=None)
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "count_bench.log"))
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    v = hsc.Validator(0)

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.log, "a") as f:
            f.write(json.dumps(row) + "\n")

    try:
        for n in a.sizes:
            for nkeys in a.keys:
                wn = n <= a.numpy_max
                if a.only != "queue":
                    emit(measure_counter(v, n, nkeys, a.repeats, wn))
                if a.only != "counter":
                    for fifo in (False, True):
                        emit(measure_queue(v, n, nkeys, fifo, a.repeats, wn))
    finally:
        v.close()


if __name__ == "__main__":
    main()
