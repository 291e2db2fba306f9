"""CPU reference of the internal-consistency entries (include/hip_serial.h,
hsc_dep_graph_internal / hsc_dep_graph_internal_lists): each
txn's ops are walked in array order with a per-key state and the rules are
applied as the header states them -- no sorting, no positions.  check_values()
and check_lists() return what Validator.graph_internal / graph_internal_lists
(arrays=True) must equal field for field (ms and sort_packed aside)."""
import numpy as np

import lists_model as LM
import resolve_model as RM
from comdb2_amd.workloads import ListHistory, ValueHistory

INIT = RM.INIT
OK, ABORTED, UNKNOWN = RM.OK, RM.ABORTED, RM.UNKNOWN
NONE = 0xFFFFFFFFFFFFFFFF  # anchor_op: unconstrained, or a write
LIST_CAP = 4096

COUNTS = ("nops", "ntxn", "checked_reads", "bad_reads", "compared_elements", "bad_txns", "n_listed")
TXN_ARRAYS = ("txn_bad", "listed_op", "listed_anchor")
OP_ARRAYS = ("bad", "anchor_op")

vh, lh = RM.vh, LM.lh


def _report(n, ntxn, txn, bad, anchor, counted, compared):
    """The report from the per-op verdicts: counted[i] = read i is constrained
    and its txn is one the counters cover."""
    txn_bad = [0] * ntxn
    listed = []
    for i in range(n):
        if counted[i] and bad[i]:
            txn_bad[txn[i]] = 1
            listed.append(i)
    out = {"nops": n, "ntxn": ntxn, "checked_reads": sum(counted), "bad_reads": len(listed),
           "compared_elements": compared, "bad_txns": sum(txn_bad), "n_listed": min(LIST_CAP, len(listed))}
    listed = listed[:LIST_CAP]
    out.update(txn_bad=np.array(txn_bad, np.uint8), listed_op=np.array(listed, np.uint64),
               listed_anchor=np.array([anchor[i] for i in listed], np.uint64), bad=np.array(bad, np.uint8),
               anchor_op=np.array(anchor, np.uint64))
    return out


def check_values(h: ValueHistory, in_c=None) -> dict:
    """in_c[t]: txn t is in the resolve's committed set (default: the resolve
    model's)."""
    txn, key, isw, val, _ = RM._cols(h)
    n = len(txn)
    if in_c is None:
        in_c = [c != RM.NO_CID for c in RM.resolve(h)["cid"]]
    last = {}  # (txn, key) -> the txn's latest op on the key
    bad, anchor, counted = [0] * n, [NONE] * n, [False] * n
    for i in range(n):
        tk = (txn[i], key[i])
        if not isw[i] and tk in last:
            anchor[i] = last[tk]
            bad[i] = int(val[i] != val[last[tk]])
            counted[i] = bool(in_c[txn[i]])
        last[tk] = i
    return _report(n, h.ntxn, txn, bad, anchor, counted, 0)


def check_lists(h: ListHistory) -> dict:
    txn, key, isw = [int(x) for x in h.txn], [int(x) for x in h.key], [int(x) for x in h.is_write]
    val, off = [int(x) for x in h.value], [int(x) for x in h.list_off]
    elems, status = [int(x) for x in h.elems], [int(x) for x in h.status]
    n = len(txn)
    state = {}  # (txn, key) -> [o_1, the latest read p or None, the elements appended since]
    bad, anchor, counted = [0] * n, [NONE] * n, [False] * n
    compared = 0
    for i in range(n):
        st = state.setdefault((txn[i], key[i]), [i, None, []])
        if isw[i]:
            st[2].append(val[i])
            continue
        first, p, A = st
        if status[txn[i]] == OK:
            mine = elems[off[i]:off[i + 1]]
            a = len(A)
            if p is not None:
                prev = elems[off[p]:off[p + 1]]
                anchor[i], counted[i] = p, True
                if len(mine) == len(prev) + a:
                    compared += len(prev) + a
                    bad[i] = int(mine != prev + A)
                else:
                    bad[i] = 1
            elif a > 0:
                anchor[i], counted[i] = first, True
                if len(mine) >= a:
                    compared += a
                    bad[i] = int(mine[len(mine) - a:] != A)
                else:
                    bad[i] = 1
        st[1], st[2] = i, []
    return _report(n, h.ntxn, txn, bad, anchor, counted, compared)


def assert_equal(res: dict, ref: dict, arrays: bool = True) -> None:
    for k in COUNTS:
        assert int(res[k]) == int(ref[k]), (k, res[k], ref[k])
    for k in TXN_ARRAYS:
        np.testing.assert_array_equal(res[k], ref[k], err_msg=k)
    for k in OP_ARRAYS:
        if arrays:
            np.testing.assert_array_equal(res[k], ref[k], err_msg=k)
        else:
            assert res[k] is None, k


def check_expected(res: dict, want: dict) -> None:
    for k, v in want.items():
        got = res[k]
        if isinstance(v, (list, tuple)):
            assert [int(x) for x in got] == list(v), (k, got, v)
        else:
            assert int(got) == v, (k, got, v)


# ---- hand-built cases: (kind, history, literal expectations) -----------------
N = NONE
HAND = {
    # value histories
    "v_write_read_equal": ("value", vh([(0, 1, "w", 1), (0, 1, "r", 1)], [OK]),
                           dict(bad=[0, 0], anchor_op=[N, 0], checked_reads=1, bad_reads=0, bad_txns=0)),
    "v_write_read_different": ("value", vh([(0, 1, "w", 1), (0, 1, "r", 5)], [OK]),
                               dict(bad=[0, 1], anchor_op=[N, 0], checked_reads=1, bad_reads=1, bad_txns=1,
                                    txn_bad=[1], listed_op=[1], listed_anchor=[0])),
    "v_read_read_different": ("value", vh([(0, 1, "r", None), (0, 1, "r", 9)], [OK]),
                              dict(bad=[0, 1], anchor_op=[N, 0], checked_reads=1, bad_reads=1)),
    "v_init_after_own_write": ("value", vh([(0, 1, "w", 1), (0, 1, "r", None)], [OK]),
                               dict(bad=[0, 1], anchor_op=[N, 0], checked_reads=1, bad_reads=1)),
    "v_init_then_init": ("value", vh([(0, 1, "r", None), (0, 1, "r", None)], [OK]),
                         dict(bad=[0, 0], anchor_op=[N, 0], checked_reads=1, bad_reads=0)),
    "v_write_write_read_first": ("value", vh([(0, 1, "w", 1), (0, 1, "w", 2), (0, 1, "r", 1)], [OK]),
                                 dict(bad=[0, 0, 1], anchor_op=[N, N, 1], checked_reads=1, bad_reads=1)),
    "v_aborted_not_counted": ("value", vh([(0, 1, "w", 1), (0, 1, "r", 5)], [ABORTED]),
                              dict(bad=[0, 1], anchor_op=[N, 0], checked_reads=0, bad_reads=0, bad_txns=0,
                                   txn_bad=[0], n_listed=0)),
    "v_dropped_unknown_not_counted": ("value", vh([(0, 1, "w", 1), (0, 1, "r", 5)], [UNKNOWN]),
                                      dict(bad=[0, 1], anchor_op=[N, 0], checked_reads=0, bad_reads=0, txn_bad=[0])),
    "v_recovered_unknown_counted": ("value", vh([(0, 1, "w", 1), (0, 1, "r", 5), (1, 1, "r", 1)], [UNKNOWN, OK]),
                                    dict(bad=[0, 1, 0], anchor_op=[N, 0, N], checked_reads=1, bad_reads=1,
                                         txn_bad=[1, 0])),
    # two txns and two keys interleaved: the anchor is the txn's own previous op on the key
    "v_interleaved": ("value", vh([(0, 1, "w", 1), (1, 1, "w", 2), (0, 2, "w", 3), (1, 1, "r", 2), (0, 1, "r", 2),
                                   (0, 2, "r", 3), (1, 1, "r", 1)], [OK, OK]),
                      dict(bad=[0, 0, 0, 0, 1, 0, 1], anchor_op=[N, N, N, 1, 0, 2, 3], checked_reads=4, bad_reads=2,
                           bad_txns=2, listed_op=[4, 6], listed_anchor=[0, 3])),
    # list histories (txn 1 appends what txn 0 finds there)
    "l_read_append_append_read": ("lists", lh([(0, 1, [5]), (0, 1, 10), (0, 1, 11), (0, 1, [5, 10, 11]), (1, 1, 5)],
                                              [OK, OK]),
                                  dict(bad=[0, 0, 0, 0, 0], anchor_op=[N, N, N, 0, N], checked_reads=1, bad_reads=0,
                                       compared_elements=3)),
    "l_read_append_append_read_swapped": ("lists", lh([(0, 1, [5]), (0, 1, 10), (0, 1, 11), (0, 1, [5, 11, 10]),
                                                       (1, 1, 5)], [OK, OK]),
                                          dict(bad=[0, 0, 0, 1, 0], anchor_op=[N, N, N, 0, N], checked_reads=1,
                                               bad_reads=1, compared_elements=3, listed_op=[3], listed_anchor=[0])),
    "l_read_append_append_read_short": ("lists", lh([(0, 1, [5]), (0, 1, 10), (0, 1, 11), (0, 1, [5, 10]), (1, 1, 5)],
                                                    [OK, OK]),
                                        dict(bad=[0, 0, 0, 1, 0], checked_reads=1, bad_reads=1, compared_elements=0)),
    "l_append_append_read_suffix": ("lists", lh([(0, 1, 10), (0, 1, 11), (0, 1, [5, 10, 11]), (1, 1, 5)], [OK, OK]),
                                    dict(bad=[0, 0, 0, 0], anchor_op=[N, N, 0, N], checked_reads=1, bad_reads=0,
                                         compared_elements=2)),
    "l_append_append_read_wrong_suffix": ("lists", lh([(0, 1, 10), (0, 1, 11), (0, 1, [5, 11, 10]), (1, 1, 5)],
                                                      [OK, OK]),
                                          dict(bad=[0, 0, 1, 0], anchor_op=[N, N, 0, N], checked_reads=1, bad_reads=1,
                                               compared_elements=2)),
    "l_append_append_read_shorter_than_a": ("lists", lh([(0, 1, 10), (0, 1, 11), (0, 1, [11])], [OK]),
                                            dict(bad=[0, 0, 1], anchor_op=[N, N, 0], checked_reads=1, bad_reads=1,
                                                 compared_elements=0)),
    "l_read_read_equal": ("lists", lh([(0, 1, [5]), (0, 1, [5]), (1, 1, 5)], [OK, OK]),
                          dict(bad=[0, 0, 0], anchor_op=[N, 0, N], checked_reads=1, bad_reads=0, compared_elements=1)),
    "l_read_read_longer": ("lists", lh([(0, 1, [5]), (0, 1, [5, 6]), (1, 1, 5), (1, 1, 6)], [OK, OK]),
                           dict(bad=[0, 1, 0, 0], anchor_op=[N, 0, N, N], checked_reads=1, bad_reads=1,
                                compared_elements=0)),
    "l_read_read_shorter": ("lists", lh([(0, 1, [5]), (0, 1, []), (1, 1, 5)], [OK, OK]),
                            dict(bad=[0, 1, 0], anchor_op=[N, 0, N], checked_reads=1, bad_reads=1,
                                 compared_elements=0)),
    "l_empty_read_after_own_append": ("lists", lh([(0, 1, 10), (0, 1, [])], [OK]),
                                      dict(bad=[0, 1], anchor_op=[N, 0], checked_reads=1, bad_reads=1,
                                           compared_elements=0, txn_bad=[1])),
    "l_first_read_unconstrained": ("lists", lh([(0, 1, [5]), (1, 1, 5)], [OK, OK]),
                                   dict(bad=[0, 0], anchor_op=[N, N], checked_reads=0, bad_reads=0,
                                        compared_elements=0)),
    "l_aborted_not_checked": ("lists", lh([(0, 1, 10), (0, 1, 11), (0, 1, [11, 10])], [ABORTED]),
                              dict(bad=[0, 0, 0], anchor_op=[N, N, N], checked_reads=0, bad_reads=0,
                                   compared_elements=0)),
    "l_unknown_not_checked": ("lists", lh([(0, 1, [5]), (0, 1, []), (1, 1, 5)], [UNKNOWN, OK]),
                              dict(bad=[0, 0, 0], anchor_op=[N, N, N], checked_reads=0, bad_reads=0)),
    # a read in the middle: the second read's prefix is the first read's list, not the appends before it
    "l_append_read_append_read": ("lists", lh([(0, 1, 10), (0, 1, [10]), (0, 1, 11), (0, 1, [10, 12])], [OK]),
                                  dict(bad=[0, 0, 0, 1], anchor_op=[N, 0, N, 1], checked_reads=2, bad_reads=1,
                                       compared_elements=3)),
}


def check(kind: str, h) -> dict:
    return check_values(h) if kind == "value" else check_lists(h)


# ---- seeded random histories ---------------------------------------------------
GPU_SEEDS = (1, 2, 3)  # tests/test_gpu_internal.py runs these; test_internal_model.py pins their coverage
_FRESH = 10 ** 12      # values / elements nobody wrote


def _interleave(rng, progs):
    """The txns' programs merged at random: every txn's ops keep their order
    and are (almost never) contiguous."""
    order = rng.permutation(np.repeat(np.arange(len(progs)), [len(p) for p in progs]))
    at = [0] * len(progs)
    ops = []
    for t in order:
        ops.append(progs[t][at[t]])
        at[t] += 1
    return ops


def _statuses(rng, n_txn):
    return rng.choice(np.array([OK, ABORTED, UNKNOWN], np.uint8), size=n_txn, p=[0.85, 0.08, 0.07])


def _keymap(rng, n_keys, full64):
    if not full64:
        return np.arange(1, n_keys + 1, dtype=np.uint64)
    return rng.integers(0, 2 ** 64, size=n_keys, dtype=np.uint64, endpoint=False)


def random_values(seed: int, n_txn: int = 2500, n_keys: int = 300, corrupt: float = 0.05,
                  full64: bool = False) -> ValueHistory:
    """About 7.5 ops a txn on one to three keys; written values are unique.  A
    constrained read returns its anchor's value, except a share ``corrupt``
    that returns a value nobody wrote, another write's value or the initial
    state."""
    rng = np.random.default_rng(seed)
    status = _statuses(rng, n_txn)
    km = _keymap(rng, n_keys, full64)
    written = {}
    nextv, fresh, progs = 1, _FRESH, []
    for t in range(n_txn):
        keys = rng.choice(n_keys, size=int(rng.integers(1, 4)), replace=False)
        last, prog = {}, []
        for _ in range(int(rng.integers(2, 14))):
            k = int(keys[int(rng.integers(0, len(keys)))])
            if rng.random() < 0.4:
                v = nextv
                nextv += 1
                written.setdefault(k, []).append(v)
                prog.append((t, int(km[k]), "w", v))
            else:
                pool = written.get(k, [])
                if k in last:
                    v = last[k]
                    if rng.random() < corrupt:
                        how = int(rng.integers(0, 3))
                        if how == 0 or (how == 1 and v is None) or (how == 2 and not pool):
                            v, fresh = fresh, fresh + 1
                        elif how == 1:
                            v = None
                        else:
                            w = pool[int(rng.integers(0, len(pool)))]
                            if w == v:
                                w, fresh = fresh, fresh + 1
                            v = w
                else:
                    v = pool[int(rng.integers(0, len(pool)))] if pool and rng.random() < 0.7 else None
                prog.append((t, int(km[k]), "r", v))
            last[k] = v
        progs.append(prog)
    return vh(_interleave(rng, progs), status)


def random_lists(seed: int, n_txn: int = 2500, n_keys: int = 16, corrupt: float = 0.05,
                 full64: bool = False) -> ListHistory:
    """A serial execution (txn t runs whole against the lists txns before it
    left; UNKNOWN txns apply half the time, ABORTED ones never), the arrays
    interleaved; appended elements are unique.  A share ``corrupt`` of the
    reads that follow an op of their txn on the key is damaged: an own append
    dropped, an own append out of place, one element of the prefix changed, or
    the list one element too short or too long."""
    rng = np.random.default_rng(seed)
    status = _statuses(rng, n_txn)
    km = _keymap(rng, n_keys, full64)
    state = {}
    nextv, fresh, progs = 1, _FRESH, []
    for t in range(n_txn):
        keys = rng.choice(n_keys, size=int(rng.integers(1, 4)), replace=False)
        work, own, touched, prog = {}, {}, set(), []
        for _ in range(int(rng.integers(2, 14))):
            k = int(keys[int(rng.integers(0, len(keys)))])
            if k not in work:
                work[k] = list(state.get(k, ()))
            if rng.random() < 0.45:
                work[k].append(nextv)
                own[k] = own.get(k, 0) + 1
                prog.append((t, int(km[k]), nextv))
                nextv += 1
            else:
                v = list(work[k])
                if k in touched and rng.random() < corrupt:
                    how, a = int(rng.integers(0, 5)), own.get(k, 0)
                    if how == 0 and a:
                        del v[len(v) - 1 - int(rng.integers(0, a))]
                    elif how == 1 and a and len(v) >= 2:
                        v[-1], v[-2] = v[-2], v[-1]
                    elif how == 2 and len(v) > a:
                        v[int(rng.integers(0, len(v) - a))] = fresh
                        fresh += 1
                    elif how == 3 and v:
                        v.pop()
                    else:
                        v.append(fresh)
                        fresh += 1
                prog.append((t, int(km[k]), v))
            touched.add(k)
        if status[t] == OK or (status[t] == UNKNOWN and rng.random() < 0.5):
            state.update(work)
        progs.append(prog)
    return lh(_interleave(rng, progs), status)
