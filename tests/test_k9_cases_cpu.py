"""K9 cases, CPU tier: what the crafted contigs of tests/k9_cases.py reach (window positions on every form switch of sel_ispr,
path lengths around the 64-edge path window, an unsettled head and a result appended where the output buffer flushes, tie runs
and conversion counts around the ballot chunk and SEL_PLAN_KEEP), and the CPU references the GPU tier
(tests/test_gpu_k9_edges.py) compares with: the emulation equals the oracle, the checker has no findings, and the emulation's
K9 counters say that the form the facts name is the form that ran.  The register form exists on the card only: no counter
can attribute it here, the facts' predicate (W <= 16, E <= 64) names its windows."""
import ctypes as C

import numpy as np
import pytest

import k9_cases as KC
import k9_checker as K
from test_k9_checker import _emul_check

KS = (KC.K_SMALL, KC.K_BIG)


@pytest.fixture(scope="module")
def CASES(T):
    names, hb = KC.batch()
    F = {}
    for Kp in KS:
        T.emul_solve(hb, Kp)
        assert T.diff_intermediates(hb, T.emul_debug, Kp) == [], Kp    # the intermediates the facts are read from are the oracle's
        F[Kp] = KC.facts(T, hb, Kp, fetch=T.emul_debug)
    got, miss = KC.coverage(names, F)
    print()
    for n in names:
        for Kp in KS:
            print("%-15s K %3d  %r" % (n, Kp, got[n][Kp]))
    return names, hb, F, got, miss


def test_the_batch_is_small(CASES):
    names, hb, F, got, miss = CASES
    N = np.diff(hb.arrays["ctg_rec_off"])
    assert len(names) < 150 and N.sum() < 20000 and N.max() <= 320


def test_coverage_misses_nothing(CASES):
    names, hb, F, got, miss = CASES
    assert miss == [], miss


def test_the_checker_has_no_findings_on_the_upgrade(CASES):
    names, hb, F, got, miss = CASES
    bad = [(Kp, n, f["bad"][:2]) for Kp, fl in F.items() for n, f in zip(names, fl) if f["bad"]]
    assert bad == [], bad[:4]


@pytest.mark.parametrize("sequential", [False, True], ids=["plan", "sequential"])
@pytest.mark.parametrize("Kp", KS, ids=lambda k: "k%d" % k)
def test_emulation_equals_the_oracle_and_the_selection_reading(T, Kp, sequential):
    names, hb = KC.batch()
    bad, out, a, per = _emul_check(T, hb, Kp, sequential)
    assert bad == [], bad[:5]
    assert T.diff_outputs(T.oracle_solve(hb, Kp), out) == []


def _k9_stats(T, reset):
    a = np.zeros(64, np.int64)
    T.emul().emul_k9_stats(a.ctypes.data_as(C.c_void_p), 1 if reset else 0)
    return dict(zip(KC.K9_STAT_NAMES, (int(x) for x in a)))


@pytest.mark.parametrize("Kp", KS, ids=lambda k: "k%d" % k)
def test_the_emulations_counters_agree_with_the_facts(T, CASES, Kp):
    """Per contig, from a one-contig solve: the DPs on the LDS copy (the register form's windows among them: the emulation serves
    them there), streamed and on global state; the settled edges; conversions and path edges."""
    names, hb, F, got, miss = CASES
    for c, (n, f) in enumerate(zip(names, F[Kp])):
        _k9_stats(T, True)
        T.emul_solve(hb.subset([c]), Kp)
        st = _k9_stats(T, True)
        ws = [w for cv in f["convs"] for w in cv["windows"] if w["called"]]
        want = dict(conversions=len(f["convs"]), path_edges=sum(cv["la"] for cv in f["convs"]), ispr_calls=len(ws), ispr_empty=0,
                    ispr_lds_dp=sum(w["form"] in ("reg", "lds") for w in ws), ispr_stream=sum(w["form"] in ("stream_narrow", "stream_wide") for w in ws),
                    ispr_generic=sum(w["form"] == "generic" for w in ws), lds_dp_window_sum=sum(w["W"] for w in ws if w["form"] in ("reg", "lds")),
                    cw_fills=sum(cv["cw_fills"] for cv in f["convs"]), edges_copied_in_runs=sum(sum(cv["runs"]) for cv in f["convs"]),
                    settled_d2=sum(cv["settled_d2"] for cv in f["convs"]), settled_d3=sum(cv["settled_d3"] for cv in f["convs"]))
        assert {k: st[k] for k in want} == want, (n, Kp)
