"""CPU model of the real-time order (hsc_dep_graph_stage_realtime, DESIGN.md
§5e), shared by test_realtime_model.py and test_gpu_realtime.py.

``full`` is the relation itself, ``reduced`` its transitive reduction read
literally (the pairs not implied by two others); ``reduced_sorted`` restates
the reduction over sorted intervals with numpy searches for the sizes at which
an n x n matrix is too large -- test_realtime_model.py checks it against
``reduced``."""
import numpy as np

OPEN = np.uint64(0xFFFFFFFFFFFFFFFF)  # HSC_RT_OPEN


def full(invoke, complete):
    """M[a, b]: a completed before b was invoked (an open a precedes nothing)."""
    invoke, complete = np.asarray(invoke, np.uint64), np.asarray(complete, np.uint64)
    return (complete != OPEN)[:, None] & (complete[:, None] < invoke[None, :])


def reduced(invoke, complete):
    """The pairs of ``full`` not implied by two others: a -> b stays unless
    some x has a -> x and x -> b."""
    m = full(invoke, complete)
    f = m.astype(np.float32)  # (path counts up to n: exact in float32)
    implied = (f @ f) > 0
    return m & ~implied


def pairs(m):
    """(src, dst) of a relation matrix, in (src, dst) order."""
    s, d = np.nonzero(m)
    return s.astype(np.uint32), d.astype(np.uint32)


def reduced_sorted(invoke, complete):
    """(src, dst) of ``reduced`` in (src, dst) order, without the matrix."""
    invoke, complete = np.asarray(invoke, np.uint64), np.asarray(complete, np.uint64)
    n = len(invoke)
    order = np.lexsort((np.arange(n), invoke))
    si, sc = invoke[order], complete[order]
    suf = np.minimum.accumulate(sc[::-1])[::-1]
    closed = np.nonzero(complete != OPEN)[0]
    p = np.searchsorted(si, complete[closed], side="right")
    has = p < n
    closed, p = closed[has], p[has]
    q = np.searchsorted(si, suf[p], side="right")
    cnt = q - p
    src = np.repeat(closed, cnt)
    pos = np.repeat(p, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    dst = order[pos]
    rows = np.sort((src.astype(np.uint64) << np.uint64(32)) | dst.astype(np.uint64))
    return (rows >> np.uint64(32)).astype(np.uint32), (rows & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def random_intervals(seed, n, procs=4, open_frac=0.0, shuffle=True, step=3):
    """n intervals of ``procs`` processes, each process one op after another
    with small integer gaps and durations (so times tie across processes and a
    completion can equal the next invoke); ``open_frac`` of the ops never
    complete (their process goes on after the moment they would have).  Txn
    ids are a random permutation unless shuffle is off (then process-major)."""
    rng = np.random.default_rng(seed)
    inv, cpl = [], []
    per = [n // procs + (1 if i < n % procs else 0) for i in range(procs)]
    for k in per:
        gap = rng.integers(0, step, size=k)
        dur = rng.integers(0, step + 2, size=k)
        end = np.cumsum(gap + dur) + int(rng.integers(0, step))
        start = end - dur
        inv.append(start)
        cpl.append(end)
    invoke = np.concatenate(inv).astype(np.uint64) if n else np.zeros(0, np.uint64)
    complete = np.concatenate(cpl).astype(np.uint64) if n else np.zeros(0, np.uint64)
    if open_frac > 0:
        complete[rng.random(n) < open_frac] = OPEN
    if shuffle:
        perm = rng.permutation(n)
        invoke, complete = invoke[perm], complete[perm]
    return invoke, complete


def merged_edges(n, *edge_sets):
    """Typed edge sets (src, dst, type) merged as the build merges them:
    parallel edges OR their types, self edges dropped; (src, dst) order."""
    rows = np.concatenate([(np.asarray(s, np.uint64) << np.uint64(32)) | np.asarray(d, np.uint64)
                           for s, d, _ in edge_sets])
    types = np.concatenate([np.broadcast_to(np.asarray(t, np.uint32), np.shape(s)) for s, _, t in edge_sets])
    keep = (rows >> np.uint64(32)) != (rows & np.uint64(0xFFFFFFFF))
    rows, types = rows[keep], types[keep]
    o = np.argsort(rows, kind="stable")
    rows, types = rows[o], types[o]
    uniq, first = np.unique(rows, return_index=True)
    t = np.bitwise_or.reduceat(types, first) if len(rows) else np.zeros(0, np.uint32)
    return ((uniq >> np.uint64(32)).astype(np.uint32), (uniq & np.uint64(0xFFFFFFFF)).astype(np.uint32),
            t.astype(np.uint32))


def remap_types(t):
    """Type words for test_anomaly.ref_anomalies / check_witnesses, whose E1
    is t & 3 and anti t == 4: the rt bit becomes a wr bit."""
    t = np.asarray(t).astype(np.int64)
    return (t & 7) | np.where(t & 8, 2, 0)
