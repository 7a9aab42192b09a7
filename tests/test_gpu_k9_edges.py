"""GPU tier, K9 on crafted contigs: the window DP's five forms (sel_ispr: registers - device-only code -, the cached LDS copy,
streamed on the narrow arrays and on the SelWide overlay, global state), the 64-edge path window, the output buffer's flush and
the plan's ballot chunks on the contigs of tests/k9_cases.py, whose windows sit on W = 15, 16 | 17, 62, 63 | 64, 65, 126, 127 |
128, 129 and 200 and whose results are not the walks' own edges.  tests/test_k9_cases_cpu.py asserts what the contigs reach.

Two batches: the contigs in order, and reversed with synth() contigs between them.  Per solve (K = 4 and 320), exactly: the
outputs against the oracle's; cv_la, both paths of every conversion, cv_n, cv_cov and mark_time against the CPU emulation's;
the checker's two halves (k9_checker.check_conversion on every conversion, batch_findings on main / alt / .all and the offsets);
the one-wave form (sequential_select, kb_select) against the three-launch form; all of it again on poisoned working memory."""
import numpy as np
import pytest

import k9_cases as KC
import k9_checker as K
from poison_testlib import BYTE_IDS, BYTES, cached, guarded, poisoned

pytestmark = pytest.mark.gpu
KS = (KC.K_SMALL, KC.K_BIG)


def _batch(T, which):
    return cached(("k9 edges", which), lambda: KC.batch() if which == "ordered" else KC.mixed(T))


def _conv_arrays(fetch, hb, Kp):
    a = K.collect(fetch, hb.arrays["ctg_rec_off"], full=True, K=Kp)
    n = len(a["cv_ctg"])
    a["cv_n"], a["cv_cov"] = fetch("cv_n", np.int32)[:n].copy(), fetch("cv_cov", np.int64)[:n].copy()
    a["mark_time"] = fetch("mark_time", np.int32)[:int(a["rec_off"][-1])].copy()
    a["walks"] = [K.conversions_of(a, c, as_arrays=True) if int(a["ctgV"][c]) else [] for c in range(hb.n_contigs)]
    return a


def _references(T, which, Kp):
    """Per (batch, K), once: the oracle's outputs and the emulation's conversion records."""
    names, hb = _batch(T, which)

    def make():
        want = T.oracle_solve(hb, Kp)
        assert T.diff_outputs(want, T.emul_solve(hb, Kp)) == []
        return want, _conv_arrays(T.emul_debug, hb, Kp)
    return cached(("k9 edges refs", which, Kp), make)


def _diff_conversions(e, a):
    """The card's conversion records against the emulation's, word for word (paths: their la / lb edges)."""
    bad = [k for k in ("conv_off", "cv_ctg", "cv_la", "cv_k", "cv_kind", "cv_ord", "cv_n", "cv_cov", "mark_time") if not np.array_equal(e[k], a[k])]
    for c, (we, wa) in enumerate(zip(e["walks"], a["walks"])):
        if len(we) != len(wa) or any(not (np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])) for x, y in zip(we, wa)):
            bad.append("walks of contig %d" % c)
    return bad


def _solve_and_compare(T, db, hb, Kp, want, emu, checker):
    res = db.solve(max_paths=Kp, keep_debug=True)
    try:
        got = res.fetch()
        a = _conv_arrays(res.debug, hb, Kp)
    finally:
        res.close()
    assert T.diff_outputs(want, got) == []
    assert _diff_conversions(emu, a) == []
    if checker:
        bad = []
        for c in range(hb.n_contigs):
            if int(a["ctgV"][c]):
                g = K.graph_of(a, c)
                for j, (pa, pb) in enumerate(K.conversions_of(a, c)):
                    bad += ["contig %d conversion %d: %s" % (c, j, x) for x in K.check_conversion(g, pa, pb)]
        assert bad == [], bad[:5]
        bad, per = K.batch_findings(got, a, hb.arrays, lambda c: a["walks"][c])
        assert bad == [], bad[:5]
    res = db.solve(max_paths=Kp, sequential_select=True)             # the whole conversion by one wave per contig (kb_select)
    try:
        assert T.diff_outputs(got, res.fetch(), stats=False) == []
    finally:
        res.close()


@pytest.mark.parametrize("which", ["ordered", "mixed"])
@pytest.mark.parametrize("Kp", KS, ids=lambda k: "k%d" % k)
def test_window_forms_on_crafted_contigs(T, Kp, which):
    names, hb = _batch(T, which)
    want, emu = _references(T, which, Kp)
    db = T.api().DeviceBatch(hb)
    try:
        _solve_and_compare(T, db, hb, Kp, want, emu, checker=True)
    finally:
        db.close()


@pytest.mark.parametrize("which", ["ordered", "mixed"])
@pytest.mark.parametrize("byte", BYTES, ids=BYTE_IDS)
def test_window_forms_on_poisoned_memory(T, byte, which):
    """Working memory filled with 0xA5 / 0xFF: a cell of the LDS copy's staging, the global DP state or the path buffers that is
    read before it is written shows in the paths, the coverages or the outputs."""
    api = T.api()
    names, hb = _batch(T, which)
    db = api.DeviceBatch(hb)
    try:
        for Kp in KS:
            want, emu = _references(T, which, Kp)
            with poisoned(api, byte):
                guarded(api, _solve_and_compare, T, db, hb, Kp, want, emu, True)
    finally:
        db.close()
