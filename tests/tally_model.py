"""CPU model of hsc_tally_check and hsc_bank_check (include/hip_serial.h,
DESIGN.md §5k): the reference's three accounting checkers restated line for
line over ``set`` and ``collections.Counter`` --

* ``set_checker``          jepsen/checker.clj:108-154
* ``total_queue_checker``  jepsen/checker.clj:163-218
* ``bank_checker``         linearizable/jepsen/src/comdb2/core.clj:152-177

-- plus the run form the entries report (a class as maximal stretches of
consecutive integers of one multiplicity) and dicts in the shape of
``Validator.tally_check`` / ``Validator.bank_check`` for the GPU tests to
compare with field by field.  Nothing here shares code with the library."""
from collections import Counter
from fractions import Fraction

import numpy as np

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
CLASSES = ("ok", "unexpected", "duplicated", "lost", "recovered")
LIST_CAP = 4096  # HSC_TALLY_LIST_CAP, HSC_BANK_LIST_CAP


def fraction(a, b):
    """checker.clj:156-161: a/b, but if b is zero, returns unity."""
    return Fraction(1) if b == 0 else Fraction(a, b)


def interval_set_str(s) -> str:
    """util.clj:483-508, the reduce over (sort set) as written."""
    runs, start, end = [], None, None
    for cur in sorted(s):
        if start is None:
            start, end = cur, cur
        elif cur == end + 1:
            end = cur
        else:
            runs.append((start, end))
            start, end = cur, cur
    if start is not None:
        runs.append((start, end))
    return "#{" + " ".join(str(a) if a == b else f"{a}..{b}" for a, b in runs) + "}"


def set_checker(attempts, adds, final_read) -> dict:
    """checker.clj:108-154.  attempts: the values of the invoke adds, adds: of
    the ok adds, final_read: the last ok read's value (None: no such read)."""
    attempts, adds = set(attempts), set(adds)
    if final_read is None:
        return {"valid": "unknown", "error": "Set was never read"}
    final_read = set(final_read)
    ok = final_read & attempts
    unexpected = final_read - attempts
    lost = adds - final_read
    recovered = ok - adds
    return {"valid": not lost and not unexpected,
            "ok": interval_set_str(ok), "lost": interval_set_str(lost),
            "unexpected": interval_set_str(unexpected), "recovered": interval_set_str(recovered),
            "ok_frac": fraction(len(ok), len(attempts)), "unexpected_frac": fraction(len(unexpected), len(attempts)),
            "lost_frac": fraction(len(lost), len(attempts)), "recovered_frac": fraction(len(recovered), len(attempts)),
            "sets": {"ok": ok, "unexpected": unexpected, "duplicated": set(), "lost": lost, "recovered": recovered}}


def total_queue_checker(attempts, enqueues, dequeues) -> dict:
    """checker.clj:163-218 over Counter as the multiset (``&`` is
    multiset/intersect, ``-`` is multiset/minus: it drops what would go
    negative)."""
    attempts, enqueues, dequeues = Counter(attempts), Counter(enqueues), Counter(dequeues)
    ok = dequeues & attempts
    unexpected = Counter({v: m for v, m in dequeues.items() if v not in attempts})
    duplicated = (dequeues - attempts) - unexpected
    lost = enqueues - dequeues
    recovered = ok - enqueues
    n = sum(attempts.values())
    ms = {"ok": ok, "unexpected": unexpected, "duplicated": duplicated, "lost": lost, "recovered": recovered}
    out = {"valid": not lost and not unexpected, "multisets": {k: +v for k, v in ms.items()}}
    for k, v in ms.items():
        out[k + "_frac"] = fraction(sum(v.values()), n)
    return out


def bank_checker(reads, n, total) -> dict:
    """core.clj:152-177 over the ok reads' balances; sums wrap to 64 bits as
    the entry's do (the reference would throw)."""
    bad = []
    for i, balances in enumerate(reads):
        if n != len(balances):
            bad.append({"type": "wrong-n", "expected": n, "found": len(balances), "op": i})
        elif total != wrap64(sum(balances)):
            bad.append({"type": "wrong-total", "expected": total, "found": wrap64(sum(balances)), "op": i})
    return {"valid": not bad, "bad_reads": bad}


def wrap64(x: int) -> int:
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def runs_of(ms) -> list:
    """A multiset (Counter, or a set: every multiplicity 1) as [(lo, hi,
    mult)]: maximal stretches of consecutive integers of one multiplicity."""
    ms = ms if isinstance(ms, Counter) else Counter(dict.fromkeys(ms, 1))
    out = []
    for v in sorted(v for v, m in ms.items() if m > 0):
        if out and out[-1][1] + 1 == v and out[-1][2] == ms[v]:
            out[-1][1] = v
        else:
            out.append([v, v, ms[v]])
    return [tuple(r) for r in out]


def tally(attempt, ack, seen, multiset=False, cap=LIST_CAP) -> dict:
    """``Validator.tally_check``'s dict (without ``ms`` and ``sort_packed``)
    from the checkers above."""
    attempt, ack, seen = ([int(v) for v in a] for a in (attempt, ack, seen))
    if multiset:
        chk = total_queue_checker(attempt, ack, seen)
        classes = chk["multisets"]
        totals = (len(attempt), len(ack), len(seen))
    else:
        chk = set_checker(attempt, ack, seen)
        classes = chk["sets"]
        totals = (len(set(attempt)), len(set(ack)), len(set(seen)))
    out = {"attempts": totals[0], "acks": totals[1], "seen": totals[2],
           "distinct": len(set(attempt) | set(ack) | set(seen)), "valid": int(chk["valid"])}
    for c in CLASSES:
        ms = classes[c]
        rs = runs_of(ms)
        count = sum(ms.values()) if isinstance(ms, Counter) else len(ms)
        k = min(len(rs), cap)
        out[c] = {"count": count, "distinct": len(ms), "runs": len(rs), "n_listed": k,
                  "lo": np.array([r[0] for r in rs[:k]], np.int64), "hi": np.array([r[1] for r in rs[:k]], np.int64),
                  "mult": np.array([r[2] for r in rs[:k]], np.uint32)}
    return out


def assert_same_tally(got: dict, want: dict) -> None:
    for k in ("attempts", "acks", "seen", "distinct", "valid"):
        assert got[k] == want[k], (k, got[k], want[k])
    for c in CLASSES:
        for k in ("count", "distinct", "runs", "n_listed"):
            assert got[c][k] == want[c][k], (c, k, got[c][k], want[c][k])
        for k in ("lo", "hi", "mult"):
            assert got[c][k].dtype == want[c][k].dtype and np.array_equal(got[c][k], want[c][k]), (c, k)


def bank(off, balance, n, total, cap=LIST_CAP) -> dict:
    """``Validator.bank_check``'s dict (without ``ms``) from bank_checker."""
    off = [int(x) for x in off]
    balance = [int(x) for x in balance]
    reads = [balance[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    chk = bank_checker(reads, n, total)
    nr = len(reads)
    kind, found = np.zeros(nr, np.uint8), np.array([wrap64(sum(r)) for r in reads], np.int64).reshape(nr)
    for b in chk["bad_reads"]:
        kind[b["op"]] = 1 if b["type"] == "wrong-n" else 2
        found[b["op"]] = b["found"]
    neg = np.array([sum(x < 0 for x in r) for r in reads], np.uint32).reshape(nr)
    bad = np.flatnonzero(kind)
    return {"n_reads": nr, "bad": len(bad), "wrong_n": int((kind == 1).sum()), "wrong_total": int((kind == 2).sum()),
            "reads_with_negative": int((neg > 0).sum()), "valid": int(chk["valid"]), "n_listed": min(len(bad), cap),
            "kind": kind, "found": found, "negatives": neg, "listed_read": bad[:cap].astype(np.uint64)}


def assert_same_bank(got: dict, want: dict) -> None:
    for k in ("n_reads", "bad", "wrong_n", "wrong_total", "reads_with_negative", "valid", "n_listed"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("kind", "found", "negatives", "listed_read"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
