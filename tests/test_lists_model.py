"""The CPU reference of the list-append entry (lists_model.py) against literal
expectations, and the generated histories the GPU tests use against what they
must contain: a GPU run that compares with the model cannot pass vacuously."""
import numpy as np
import pytest

import lists_model as M
from comdb2_amd import hsc
from test_anomaly import ref_anomalies
from si_model import ref_si


def check_expected(res, want):
    M.check_expected(res, want)


@pytest.mark.parametrize("name", sorted(M.HAND))
def test_hand_built(name):
    h, want = M.HAND[name]
    check_expected(M.resolve(h), want)


@pytest.mark.parametrize("name", sorted(M.INVALID))
def test_invalid(name):
    with pytest.raises(ValueError):
        M.resolve(M.INVALID[name])


def test_flag_values_match_the_binding():
    assert (M.A, M.B, M.D, M.I) == (hsc.RD_ABORTED, hsc.RD_INTERMEDIATE, hsc.RD_DANGLING, hsc.RD_INTERNAL)
    assert (M.X, M.U) == (hsc.LRD_INCOMPATIBLE, hsc.LRD_DUPLICATE)
    assert M.LIST_CAP == hsc.RESOLVE_LIST_CAP
    assert set(M.COUNTS) == set(hsc.LRESOLVED_COUNTERS)


def classes_of(oracle_mod, ref):
    s, d, t = ref["edges"]
    return ref_anomalies(oracle_mod, ref["ncommitted"], s, d, t)


def ww_only_cycle(oracle_mod, ref):
    s, d, t = (a.astype(np.int64) for a in ref["edges"])
    ww = (t & M.WW) != 0
    scc = oracle_mod.scc(ref["ncommitted"], s[ww], d[ww])
    return bool((np.bincount(scc, minlength=ref["ncommitted"]) > 1).any())


# Elle's textbook anomalies as list-append histories: the class of the one component
@pytest.mark.parametrize("name,cls,nonadj", [("g0", 1, 1), ("g1c", 1, 1), ("gsingle", 2, 1), ("g2", 4, 0),
                                             ("write_skew", 4, 0)])
def test_textbook_classes(oracle_mod, name, cls, nonadj):
    ref = M.resolve(M.HAND[name][0])
    an = classes_of(oracle_mod, ref)
    assert an.comp_class.tolist() == [cls]
    s, d, t = ref["edges"]
    si = ref_si(oracle_mod, ref["ncommitted"], s, d, t)
    assert si.comp_nonadj.tolist() == [nonadj]  # write skew is legal under snapshot isolation
    assert ww_only_cycle(oracle_mod, ref) == (name == "g0")


def test_permuted_ids_change_nothing_but_names():
    h, _ = M.HAND["g1a"]
    a, b = M.resolve(h), M.resolve(M.permuted(h, 3))
    for k in M.COUNTS:
        assert a[k] == b[k], k
    np.testing.assert_array_equal(a["rflag"], b["rflag"])


@pytest.mark.parametrize("name", sorted(M.GEN_CASES))
def test_generated_holds_every_flag_and_class(oracle_mod, name):
    h, ref = M.gen_case(name)
    for k in ("g1a_reads", "g1b_reads", "dangling_reads", "duplicate_reads", "incompatible_reads", "internal_reads",
              "recovered", "dropped", "aborted", "unobserved_appends", "ww", "wr", "rw", "incompatible_keys"):
        assert ref[k] > 0, k
    for bit in (M.A, M.B, M.D, M.I, M.X, M.U):
        assert (ref["rflag"] & bit).any(), bit
    an = classes_of(oracle_mod, ref)
    assert {1, 2, 4} <= set(an.comp_class.tolist())
    assert ww_only_cycle(oracle_mod, ref)
    # ids are in no order: some ww edge goes down in id
    s, d, t = ref["edges"]
    assert ((t & M.WW != 0) & (s > d)).any()
    if name == "full64":
        assert int(h.key.max()) > 2 ** 63 and int(h.elems.max()) > 2 ** 63
