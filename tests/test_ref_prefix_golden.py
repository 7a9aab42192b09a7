"""K1 ... K8 against vectors recorded from the REAL reference (no /root/reference needed at run time).

tests/golden/ref_prefix.npz holds input batches and, per contig, the locals of the reference's own solve_ctg_read()
at paf_data.cpp:738 - sorted order, part ids, every (i, j) cut of the N x N tables, vertex ids, adjacency order with
all weight fields, anom_dis[dest], d / best, both Kahn orders, every sidetrack-heap node and root, the k-walk
distances - recorded by tests/golden/make_ref_prefix.py from oracle/_ref/libaasm_ref_prefix_mono.so (the reference's
lines compiled in place; oracle/Makefile).  Checked against them here:
  CPU tier: the oracle (so "HIP == oracle" elsewhere means "== reference" for these stages) and the product's
            kernel bodies in the 1-lane emulation;
  GPU tier: the HIP kernels' intermediates on the card, at K = 10 000 and at small K, with either K7 kernel.
tests/golden/ref_prefix_overhang.npz holds the same for batches of tests/overhang_cases.py (records that run to or past the
query's end: negative dest edges and walk sums), tests/golden/ref_prefix_enum.npz for the crafted contigs of tests/enum_cases.py
(walk-sum distributions chosen on purpose, all in one batch); every check here runs over the three files - one body per check, a
test per file (the first file's tests keep their names)."""
import os

import numpy as np
import pytest

HIP_FORMS = [("auto", "auto"), ("all", "auto"), ("none", "auto"), ("auto", "none"), ("auto", "half")]


@pytest.fixture(scope="module")
def V(T):
    return T.RefPrefixVectors()


@pytest.fixture(scope="module")
def VO(T):
    return T.RefPrefixVectors(os.path.join(T.GOLDEN, "ref_prefix_overhang.npz"))


@pytest.fixture(scope="module")
def VE(T):
    return T.RefPrefixVectors(os.path.join(T.GOLDEN, "ref_prefix_enum.npz"))


def test_fixture_covers_the_stages(T, V):
    assert len(V.tags) >= 15
    n_pairs = n_nodes = n_dist = n_nsl = 0
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        n_nsl += nsl
        for c in range(hb.n_contigs):
            r = V.contig(tag, c)
            if r:
                assert set(T.PREFIX_NAMES) <= set(r)
                n_pairs += len(r["pair_pe_q"]); n_nodes += int(r["heap_nodes"][0]); n_dist += len(r["kd_qry"])
    assert n_pairs > 2000 and n_nodes > 100000 and n_dist > 100000 and n_nsl >= 4


def test_overhang_fixture_holds_its_input_class(T, VO):
    """What the reference itself computed on the overhang batches: dest edges below zero, contigs whose recorded walks are all
    negative, contigs whose 10 000 walks cross zero, and negative sums spread over more than 50 000 in one contig."""
    V = VO
    assert len(V.tags) >= 7
    n_neg_edges = n_all_neg = n_cross = n_dist = n_nsl = n_touch = spread = 0
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        assert (np.diff(hb.arrays["ctg_rec_off"]) <= 30).all() or hb.n_contigs == 1
        n_nsl += nsl
        for c in range(hb.n_contigs):
            r = V.contig(tag, c)
            if not r:
                continue
            assert set(T.PREFIX_NAMES) <= set(r)
            s = r["kd_qry"] + r["kd_ref"]
            n_dist += len(s); n_neg_edges += int((r["csr_w_qry"] < 0).sum()); n_touch += int(r["csr_w_qry"].min() == 0)
            n_all_neg += bool((s < 0).all()); n_cross += bool(s.min() < 0 <= s.max())
            if full and (s < 0).all():
                spread = max(spread, int(s.max() - s.min()))
    assert n_neg_edges > 300 and n_all_neg >= 10 and n_cross >= 3 and n_touch >= 6 and n_dist > 50000 and n_nsl >= 1 and spread > 50000


def test_enum_fixture_holds_the_crafted_contigs(T, VE):
    """The recorded batch IS enum_cases.contigs() (tests/test_gpu_enum_edges.py checks the card against these vectors by contig
    index), every contig is recorded, and the reference's own distances show the distributions: one sum, all sums distinct,
    groups of ties, sums below zero."""
    import enum_cases as EC
    names, hb = EC.batch(EC.contigs())
    assert VE.tags == ["enum"]
    rec, nsl, full = VE.batch("enum")
    assert full and not nsl and set(rec.arrays) == set(hb.arrays)
    for k in hb.arrays:
        assert np.array_equal(rec.arrays[k], hb.arrays[k]), k
    R = {n: VE.contig("enum", c) for c, n in enumerate(names)}
    assert all(set(T.PREFIX_NAMES) <= set(r) for r in R.values())
    sums = {n: r["kd_qry"] + r["kd_ref"] for n, r in R.items()}
    assert len(sums["all_equal"]) == 4096 and len(np.unique(sums["all_equal"])) == 1
    assert len(sums["all_equal_big"]) == 10000 and R["all_equal_big"]["kfound"][0] == 10000 and len(np.unique(sums["all_equal_big"])) == 1
    assert len(np.unique(sums["all_distinct"])) == 4096 and len(np.unique(sums["clusters"])) == 4
    assert len(sums["negative_ties"]) == 1024 and (sums["negative_ties"] < 0).all() and len(np.unique(sums["negative_ties"])) == 4
    assert len(np.unique(R["anom_split"]["kd_anom"])) == 6 and len(np.unique(sums["anom_split"])) == 1
    assert [len(sums[n]) for n in ("chain", "few_2", "few_3", "few_4", "few_5")] == [1, 2, 3, 4, 5]


def test_oracle_matches_recorded_reference_prefix(T, V):
    _oracle_matches(T, V)


def test_oracle_matches_recorded_reference_prefix_overhang(T, VO):
    _oracle_matches(T, VO)


def test_oracle_matches_recorded_reference_prefix_enum(T, VE):
    _oracle_matches(T, VE)


def _oracle_matches(T, V):
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        for c in range(hb.n_contigs):
            r = V.contig(tag, c)
            if not r:
                continue
            o = T.oracle_debug(hb, c, 10000, nsl)
            assert len(o["kd_qry"]) == r["kfound"][0], (tag, c)
            for n in T.PREFIX_NAMES:
                want = r[n]
                assert np.array_equal(o[n][:len(want)] if n.startswith("kd_") else o[n], want), (tag, c, n)


def test_kernel_bodies_match_recorded_reference_prefix_enum(T, VE):
    _kernel_bodies_match(T, VE)


def test_kernel_bodies_match_recorded_reference_prefix(T, V):
    _kernel_bodies_match(T, V)


def test_kernel_bodies_match_recorded_reference_prefix_overhang(T, VO):
    _kernel_bodies_match(T, VO)


def _kernel_bodies_match(T, V):
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        for K in ((10000, 4) if full else (64,)):
            T.emul_solve(hb, K, nsl)
            assert T.diff_intermediates(hb, T.emul_debug, K, nsl, expect=lambda c: V.contig(tag, c)) == [], (tag, K)


@pytest.mark.gpu
@pytest.mark.parametrize("heap_waves,chain", HIP_FORMS)
def test_hip_intermediates_match_recorded_reference_prefix(T, V, heap_waves, chain):
    _hip_intermediates_match(T, V, heap_waves, chain)


@pytest.mark.gpu
@pytest.mark.parametrize("heap_waves,chain", HIP_FORMS)
def test_hip_intermediates_match_recorded_reference_prefix_overhang(T, VO, heap_waves, chain):
    _hip_intermediates_match(T, VO, heap_waves, chain)


@pytest.mark.gpu
@pytest.mark.parametrize("heap_waves,chain", HIP_FORMS)
def test_hip_intermediates_match_recorded_reference_prefix_enum(T, VE, heap_waves, chain):
    _hip_intermediates_match(T, VE, heap_waves, chain)


def _hip_intermediates_match(T, V, heap_waves, chain):
    """The HIP path's intermediates on the card against what the reference's own statements computed - with either K7 kernel
    forced, and with the sparse contigs in the chain class (aasm_k67_chain; the default for batches this small), in the three
    launches, or split between the two."""
    api = T.api()
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        db = api.DeviceBatch(hb)
        for K in ((10000, 4) if full else (64, 1)):
            res = db.solve(max_paths=K, non_skip_linkable=nsl, keep_debug=True, heap_waves=heap_waves, chain=chain)
            bad = T.diff_intermediates(hb, res.debug, K, nsl, expect=lambda c: V.contig(tag, c))
            res.close()
            assert bad == [], (tag, K, bad[:6])
        db.close()
