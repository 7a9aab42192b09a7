"""Enumeration cases, CPU tier: what the crafted contigs of tests/enum_cases.py are, and the CPU references the GPU tier
(tests/test_gpu_enum_edges.py) compares the sorted-runs queue with.

K8's shipped queue (kb_enum_lsm, alignasm_amd/csrc/aasm_enum.h) exists only on the card; what it does is decided by the distribution
of the walks' score sums.  Here every distribution the contigs are named for is asserted from the oracle's walks and from the
emulation's klast / kcand records (enum_cases.coverage), and the emulation (the d-ary heap form) is checked against the oracle
at the K values that sit on the walk counts - so the inputs, and the klast / kcand reference, are pinned without a GPU."""
import numpy as np
import pytest

import enum_cases as EC

FEW = {"few_2": 2, "few_3": 3, "few_4": 4, "few_5": 5}


@pytest.fixture(scope="module")
def COV(T):
    cov = EC.coverage(T)
    print()
    for n, f in cov.items():
        print("%-14s records %2d  W %5d  distinct sums %4d  anoms %2d  ratios %d  far pops %4d  far pushes %4d  peak pending %4d  scans %4d  most near in one scan %4d"
              % (n, f["N"], f["W"], f["distinct"], len(f["anoms"]), len(f["ratios"]), f["far_pops"], f["far_pushes"], f["peak"], f["scans"], f["scan_near"]))
    return cov


def test_every_contig_is_small_and_measured_exactly(COV):
    assert [n for n, _, _ in EC.contigs()] == list(COV)
    for n, f in COV.items():
        assert f["N"] < 40, n
        assert f["peak_exact"] and f["K"] == f["W"] + 1 and f["pushes"] == f["W"] - 1, n       # every walk but the first is one push


def test_all_equal(COV):
    """One sum, one anom, one ratio: node:index decides every compare, T never moves, nothing goes far.  With every key tied the
    smallest heap node pops first, and heap nodes are numbered from dest outwards (the heap wave's BFS order of the SP tree),
    so a popped entry's successors pop before its waiting siblings: the enumeration is depth-first, and fewer entries wait at
    once than the contig has records - the front alone holds them (equal_deep is the equal-sum contig that fills the runs)."""
    for n, W in (("all_equal", 4096), ("all_equal_big", 16384)):
        f = COV[n]
        assert f["W"] == W and f["distinct"] == 1 and len(f["anoms"]) == 1 and len(f["ratios"]) == 1, n
        assert f["far_pops"] == 0 and f["far_pushes"] == 0 and f["scans"] == 0, n
        assert 1 < f["peak"] <= f["N"], n
    assert COV["all_equal_big"]["W"] >= 10000


def test_equal_deep(COV):
    f = COV["equal_deep"]
    assert f["W"] == 6561 and f["distinct"] == 1 and len(f["anoms"]) == 1
    assert f["far_pops"] == 0 and f["far_pushes"] == 0 and f["scans"] == 0
    assert f["peak"] > 1000


def test_ratio_only(COV):
    f = COV["ratio_only"]
    assert f["W"] == 2187 and f["distinct"] == 1 and len(f["anoms"]) == 1 and len(f["ratios"]) >= 6
    assert f["far_pops"] == 0
    assert f["peak"] > 64                                  # past the front: tied sums and anoms are ordered by key2 in I and the runs too


def test_all_distinct(COV):
    f = COV["all_distinct"]
    assert f["W"] == 4096 and f["distinct"] == 4096
    assert f["far_pops"] >= f["W"] - 2 and f["far_pushes"] >= f["W"] - 2
    assert f["scans"] >= f["W"] - 2 and f["peak"] > 1000


def test_clusters(COV):
    f = COV["clusters"]
    u, cnt, gaps = EC.groups(f["sums"])
    assert len(u) >= 3 and (cnt >= 200).all()              # groups of equal sums: a group's spread is 0 ...
    assert (gaps > 0).all()                                # ... and neighbouring groups are apart
    assert f["scans"] == len(u) - 1
    assert f["scan_near"] > 64                             # one scan brings more than I holds near at once


def test_geometric(COV):
    f = COV["geometric"]
    u, cnt, gaps = EC.groups(f["sums"])
    g = np.unique(gaps)
    assert len(g) >= 10 and (g[1:] >= 2 * g[:-1]).all(), g
    assert f["far_pops"] > 1000


def test_small_far(COV):
    f = COV["small_far"]
    assert f["W"] >= 100 and 0 < f["far_pushes"] < 64 and f["far_pops"] > 0
    assert 0 < f["scan_near"] < 64


def test_few_walks(COV):
    for n, W in FEW.items():
        assert COV[n]["W"] == W and COV[n]["pushes"] == W - 1, n
    f = COV["chain"]
    assert f["W"] == 1 and f["pushes"] == 0 and f["peak"] == 0


def test_negative_ties(T, COV):
    f = COV["negative_ties"]
    names, hb = EC.batch(EC.contigs())
    c = names.index("negative_ties")
    off = hb.arrays["ctg_rec_off"]
    qs, qe, qt = (hb.arrays[k][off[c]:off[c + 1]] for k in ("qry_str", "qry_end", "qry_total"))
    last = qs == qs.max()
    assert last.sum() >= 2 and (qe[last] >= qt[last] - 1).all()          # the last stage runs to or past the query's end
    u, cnt, gaps = EC.groups(f["sums"])
    assert f["W"] >= 500 and (f["sums"] < 0).all() and (cnt > 1).any() and len(u) > 1
    assert f["far_pops"] > 0


def test_anom_split(COV):
    f = COV["anom_split"]
    assert f["distinct"] == 1 and len(f["anoms"]) >= 2 and len(f["ratios"]) == 1 and f["W"] >= 500


# ---- the emulation (heap form) against the oracle, at the K values that sit on the walk counts ------------------------------------
def _check(T, hb, K):
    want = T.oracle_solve(hb, K)
    got, runs = EC.emul_enum(T, hb, K)
    assert T.diff_outputs(want, got) == [], K
    assert T.diff_intermediates(hb, T.emul_debug, K) == [], K
    return runs


@pytest.mark.parametrize("K", [1, 64, 65, 10000])
def test_emulation_matches_the_oracle_on_the_whole_batch(T, K):
    names, hb = EC.batch(EC.contigs())
    runs = _check(T, hb, K)
    for c, (found, kd, klast, cand) in enumerate(runs):
        EC.replay(T.oracle_debug(hb, c, K), found, klast, cand)            # the kcand records are the heap arrays' successors


@pytest.mark.parametrize("name", [n for n, _, _ in EC.contigs()])
def test_emulation_matches_the_oracle_around_the_walk_count(T, COV, name):
    names, hb = EC.batch(EC.contigs())
    one = hb.subset([names.index(name)])
    W = COV[name]["W"]
    for K in (W - 1, W, W + 1):
        if K < 1:
            continue
        found, kd, klast, cand = _check(T, one, K)[0]
        assert found == min(K, W)
        EC.replay(T.oracle_debug(one, 0, K), found, klast, cand)


def test_a_smaller_k_bounds_the_pending_count_from_above(T, COV):
    """facts() at K < pushes counts pushes that the kernel may cut or drop: its peak is reported as an upper bound (and, being that
    of the first K pops of the full run, it never exceeds the exact one)."""
    names, hb = EC.batch(EC.contigs())
    one = hb.subset([names.index("equal_deep")])
    f = EC.facts(T, one, 0, 2000)
    assert not f["peak_exact"] and f["far_pushes"] is None and f["K"] == 2000
    assert 64 < f["peak"] <= COV["equal_deep"]["peak"]


# ---- the real reference ---------------------------------------------------------------------------------------------------
@pytest.mark.ref
def test_oracle_matches_reference_prefix_on_the_crafted_contigs(T):
    if T.ref_prefix(True) is None:
        pytest.skip("oracle/_ref/libaasm_ref_prefix*.so not built (no reference sources on this machine and no prebuilt .so)")
    from test_ref_prefix import _diff_oracle
    names, hb = EC.batch(EC.contigs())
    bad, nd, _ = _diff_oracle(T, hb, range(hb.n_contigs), False)
    assert bad == [], bad[:6]
    assert nd > 30000
