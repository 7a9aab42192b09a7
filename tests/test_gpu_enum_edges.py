"""GPU tier, K8 on crafted walk-sum distributions: the sorted-front / sorted-runs / far-tier queue (kb_enum_lsm<64> and <40>,
alignasm_amd/csrc/aasm_enum.h - device-only code) on the contigs of tests/enum_cases.py.

What that queue does follows from how a contig's walk sums are distributed, and here the distribution is chosen: all sums equal
(every compare falls through to key2 or node:index, T never moves, the far tier stays empty - with a handful or with more than
1 000 entries waiting), all sums distinct (every push but the first goes far, one scan per pop), groups of ties that come near
1 024 at once (I overflows inside eq_redistribute), geometric gaps, fewer than 64 far entries (the n < 64 sample), ties on the
sum with different ratios or anoms, sums below zero (QE_SUM_BIAS), and 1 ... 5 walks.  tests/test_enum_cases_cpu.py asserts
that the contigs are what they are named for.

K sits on the steps of enum_k64 / enum_lmax (64 -> lmax 0, 65 -> 1, 129 -> 2, 4 097 -> 7), on both sides of KN_ENUM_S's K > 21,
at the contigs' walk counts W - 1, W, W + 1 (runs cut at K - found, the bound that drops pushes, the queue running empty exactly
at K), and at 3 W + 1 of the largest contig, where nothing is ever cut.  Two batches: the contigs in order, and reversed with
synth() contigs between them, so that every queue's neighbours in `pq` change and are checked.

Per solve, exactly: kfound and all five fields of every popped distance against the oracle and against the vectors recorded from
the reference (tests/golden/ref_prefix_enum.npz); the outputs against the oracle's; klast[:kfound] and the (heap node,
predecessor) of every kcand record up to the last popped one against the CPU emulation's of the same K; the three forms against
each other (test_gpu_enum.check_queue_forms)."""
import os

import pytest

import enum_cases as EC
from poison_testlib import BYTE_IDS, BYTES, cached, solve_checked
from test_gpu_enum import check_queue_forms

pytestmark = pytest.mark.gpu

W_ = {"all_equal": 4096, "all_distinct": 4096, "clusters": 4096, "ratio_only": 2187}        # asserted in tests/test_enum_cases_cpu.py
K_STEPS = (1, 2, 22, 63, 64, 65, 127, 128, 129, 4096, 4097, 10000)
K_WALKS = tuple(sorted({w + d for w in W_.values() for d in (-1, 0, 1)} - set(K_STEPS)))   # 2 186, 2 187, 2 188, 4 095
K_UNCUT = 3 * 16384 + 1                                                                       # all_equal_big: the most walks
KS = K_STEPS + K_WALKS + (K_UNCUT,)


def _batch(T, which):
    return cached(("enum edges", which), lambda: EC.batch(EC.contigs()) if which == "ordered" else EC.mixed(T))


def _references(T, which, K):
    """Per (batch, K), once: the oracle's outputs and per-contig intermediates, and the emulation's klast / kcand."""
    names, hb = _batch(T, which)

    def make():
        want = T.oracle_solve(hb, K)
        dbg = [T.oracle_debug(hb, c, K) for c in range(hb.n_contigs)]
        got, runs = EC.emul_enum(T, hb, K)
        assert T.diff_outputs(want, got) == []
        return want, dbg, runs
    return cached(("enum edges refs", which, K), make)


def test_the_walk_counts_the_k_values_sit_on(T):
    names, hb = _batch(T, "ordered")
    for n, w in W_.items():
        assert len(T.oracle_debug(hb, names.index(n), EC.K_ALL)["kd_qry"]) == w, n
    most = max(len(T.oracle_debug(hb, c, EC.K_ALL)["kd_qry"]) for c in range(hb.n_contigs))
    assert K_UNCUT >= 3 * most + 1
    assert len(KS) == len(set(KS)) == 17


@pytest.mark.parametrize("which", ["ordered", "mixed"])
@pytest.mark.parametrize("K", KS, ids=lambda k: "k%d" % k)
def test_queue_forms_on_crafted_distributions(T, K, which):
    names, hb = _batch(T, which)
    want, dbg, runs = _references(T, which, K)
    recorded = None
    if which == "ordered" and K <= 10000:                          # (the reference's own K is 10 000; the fixture holds this very batch)
        V = cached("enum edges vectors", lambda: T.RefPrefixVectors(os.path.join(T.GOLDEN, "ref_prefix_enum.npz")))
        recorded = lambda c: V.contig("enum", c)
    check_queue_forms(T, hb, K, expect=lambda c: dbg[c], want=want, emul=runs, recorded=recorded)


@pytest.mark.parametrize("byte", BYTES, ids=BYTE_IDS)
def test_runs_forms_on_poisoned_memory(T, byte):
    """The two runs forms on working memory filled with 0xA5 / 0xFF, at K one past a front (lmax 1) and one past 4 096 (lmax 7):
    a cell of `pq`, the far tier or the LDS slots that is read before it is written shows in the distances or the outputs."""
    names, hb = _batch(T, "ordered")
    db = T.api().DeviceBatch(hb)
    try:
        for K in (65, 4097):
            for hooks in ({}, dict(enum_small=True)):
                solve_checked(T, "enum edges", hb, K, byte, db=db, **hooks)
    finally:
        db.close()
