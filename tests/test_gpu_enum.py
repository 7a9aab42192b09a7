"""GPU tier, K8 (k_shortest_walks.hpp:217-249): the sorted-front / sorted-runs queue (aasm_enum.h) against the oracle AND
against the d-ary heap form of the same kernel - every popped distance, the insertion index of every pop, and the
(heap node, predecessor) record of every push, at K large enough that the insertion buffer is flushed, runs are merged
down several levels, cut at K - found, and the front is refilled from the run heads many times.  (These are synth() batches;
tests/test_gpu_enum_edges.py runs the same check on walk-sum distributions chosen on purpose.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

#        contigs, records, seed, K, dense, dup_every
CASES = [(3, 1000, 21, 10000, False, 0),     # the bench's k10000 shape
         (2, 400, 31, 10000, True, 0),       # dense: hundreds of distinct sums, deep heaps
         (3, 1000, 5, 2500, False, 3),       # ties from duplicated records
         (4, 600, 9, 70, False, 0),          # K just past one front (64)
         (4, 600, 9, 64, False, 0),
         (4, 600, 9, 200, True, 0),
         (2, 1000, 3, 1000, False, 0),
         (6, 30, 4, 10000, False, 0),        # tiny graphs: the queue runs empty long before K
         (1, 3000, 8, 30000, False, 0)]      # more levels (lmax = 9)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%dx%d_s%d_k%d_%s%s" % (c[0], c[1], c[2], c[3], "D" if c[4] else "S", "_dup%d" % c[5] if c[5] else ""))
def test_enumeration_queue_forms_agree_with_each_other_and_the_oracle(T, case):
    nc, nr, seed, K, dense, dup = case
    check_queue_forms(T, T.synth(nc, nr, seed, dense=dense, dup_every=dup), K)


def check_queue_forms(T, hb, K, expect=None, want=None, emul=None, recorded=None):
    """The three queue forms of K8 on one batch (tests/test_gpu_overhang.py and tests/test_gpu_enum_edges.py call this too).
    `expect(c)`: the oracle's intermediates of contig c where the caller has them already; `want`: T.oracle_solve(hb, K) likewise;
    `emul`: enum_cases.emul_enum's per-contig (kfound, kd, klast, kcand rows) of an emulated solve at the same K - every form's
    klast[:kfound] and kcand[:last popped index + 1] (heap node, predecessor) must equal the CPU emulation's;
    `recorded(c)`: vectors recorded from the reference for contig c (or {}), checked like the oracle's."""
    nc = hb.n_contigs
    api = T.api()
    db = api.DeviceBatch(hb)
    got = {}
    if expect is None:
        memo = {}

        def expect(c):                                               # (one oracle run per contig for the three forms)
            if c not in memo:
                memo[c] = T.oracle_debug(hb, c, K)
            return memo[c]
    for form in ("runs", "runs40", "heap"):                          # 64-entry front, the 40-entry front of big batches, the d-ary heap
        res = db.solve(max_paths=K, keep_debug=True, enum_heap=(form == "heap"), enum_small=(form == "runs40"))
        kf = res.debug("kfound", np.int32)[:nc].copy()
        kd = res.debug("kd", T.DIST_DT)[:nc * K].copy()
        klast = res.debug("klast", np.int32)[:nc * K].copy()
        S = 3 * K + 1
        cand = res.debug("kcand", np.int32)[:nc * S * 8].reshape(nc * S, 8)    # {heap node, predecessor, qry (2 words)}, {anom, qnz, qtot, -}
        knodes, kprev = cand[:, 0].copy(), cand[:, 1].copy()
        got[form] = (kf, kd, klast, knodes, kprev, res.fetch())
        assert T.diff_intermediates(hb, res.debug, K, expect=expect) == [], form     # kfound + every popped distance vs the oracle
        if recorded is not None:
            have = [c for c in range(nc) if recorded(c)]
            assert T.diff_intermediates(hb, res.debug, K, contigs=have, expect=recorded) == [], form
        res.close()
    db.close()
    for other in ("heap", "runs40"):
        a, b = got["runs"], got[other]
        assert np.array_equal(a[0], b[0]), other
        for c in range(nc):
            n = int(a[0][c])
            assert n >= 1
            for f in ("qry", "ref", "anom", "qnz", "qtot"):
                assert np.array_equal(a[1][f][c * K:c * K + n], b[1][f][c * K:c * K + n]), (other, c, f)
            assert np.array_equal(a[2][c * K:c * K + n], b[2][c * K:c * K + n]), (other, c)
            S = 3 * K + 1
            pushed = int(a[2][c * K:c * K + n].max()) + 1            # every push up to the last popped one was numbered alike
            assert np.array_equal(a[3][c * S:c * S + pushed], b[3][c * S:c * S + pushed]), (other, c)
            assert np.array_equal(a[4][c * S:c * S + pushed], b[4][c * S:c * S + pushed]), (other, c)
        assert T.diff_outputs(a[5], b[5]) == [], other
    want = want if want is not None else T.oracle_solve(hb, K)
    for form in got:
        assert T.diff_outputs(want, got[form][5]) == [], form
    if emul is not None:
        S = 3 * K + 1
        for form, (kf, kd, klast, knodes, kprev, _) in got.items():
            for c in range(nc):
                found, ekd, eklast, ecand = emul[c]
                assert int(kf[c]) == found, (form, c)
                assert np.array_equal(klast[c * K:c * K + found], eklast), (form, c, "klast")
                pushed = int(eklast.max()) + 1 if found else 0
                assert np.array_equal(knodes[c * S:c * S + pushed], ecand[:pushed, 0]), (form, c, "kcand node")
                assert np.array_equal(kprev[c * S:c * S + pushed], ecand[:pushed, 1]), (form, c, "kcand predecessor")


def test_queue_forms_agree_on_mixed_batches_and_many_k(T):
    """Heavy-tailed, dense and duplicate-heavy contigs at K around the front's capacity (22, 65, 130) and above: the two front
    capacities of the sorted-runs queue against the d-ary heap form (tools/k8_stress.py runs the long version)."""
    api = T.api()
    n_checked = 0
    for seed, nc, nr, dense, dup, heavy in ((1, 40, 300, False, 0, True), (3, 16, 220, True, 0, False), (4, 30, 120, True, 2, True)):
        hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup, heavy_tail=heavy)
        db = api.DeviceBatch(hb)
        for K in (22, 65, 130, 2500):
            got = {}
            for form in ("heap", "runs", "runs40"):
                res = db.solve(max_paths=K, keep_debug=True, enum_heap=(form == "heap"), enum_small=(form == "runs40"))
                got[form] = (res.debug("kfound", np.int32)[:nc].copy(), res.debug("kd", T.DIST_DT)[:nc * K].copy(), res.debug("klast", np.int32)[:nc * K].copy())
                res.close()
            for other in ("runs", "runs40"):
                a, b = got["heap"], got[other]
                assert np.array_equal(a[0], b[0]), (seed, K, other)
                for c in range(nc):
                    n = int(a[0][c])
                    assert np.array_equal(a[1][c * K:c * K + n], b[1][c * K:c * K + n]) and np.array_equal(a[2][c * K:c * K + n], b[2][c * K:c * K + n]), (seed, K, other, c)
                    n_checked += 1
        db.close()
    assert n_checked == 2 * 4 * (40 + 16 + 30)
