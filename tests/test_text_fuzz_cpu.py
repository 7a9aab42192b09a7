"""CPU tier of the text fuzz (tests/text_fuzz.py): every adversarial text through the host reader + emulated solve, K0 in the
emulation, the emulated device reader, the walking writer and the planned writer on emulated cut plans, against the oracle side
alone (I/O oracle reader -> solver oracle -> I/O oracle writers, whose get_edited_paf_data carries the reference's own
consistency throw).  What the corpora must contain is asserted on the oracle's output and on plans that were first checked against
it, so a generator gone quiet cannot hide a failure."""
import ctypes as C
import os

import numpy as np
import pytest

import cuts_testlib as X
import read_testlib as XR
import text_fuzz as F
from alignasm_amd import _abi

N_TEXTS = 36                                                         # x 2 (K, nsl) runs = 72 runs per corpus; about 4 s per corpus


@pytest.fixture(scope="module")
def emc():
    return X.build_emul()


@pytest.fixture(scope="module")
def emr():
    return XR.build_emul()


def emul_k0_solve(T, view, K, nsl):
    """The emulated solve on a batch in its cs form: K0 makes the match ranges."""
    out = _abi.BatchOut()
    rc = T.emul().emul_solve_batch(C.byref(view), C.byref(_abi.make_opts(K, nsl, 0, False, True)), C.byref(out))
    assert rc == 0, rc
    try:
        return _abi.unpack_out(out)
    finally:
        T.emul().emul_free_out(C.byref(out))


def plan_flags_equal_verdict(plans, exp):
    for k in X.LISTS:
        got = [int(f) & _abi.AASM_CUT_ERRORS for f in plans[k]["flags"]]
        assert got == exp.verdict[k], k


def writers_fail_cleanly(api, paf, bo, plans, exp, d, stem):
    """Both writers refuse the file with the oracle's text and leave nothing behind."""
    for what, cuts in (("walk", None), ("plan", plans)):
        with pytest.raises(api.AlignasmError) as e:
            X.write_three(paf, bo, d, "%s_%s" % (stem, what), cuts=cuts)
        assert e.value.code == _abi.AASM_E_PARSE and exp.message in str(e.value), what
    assert [f for f in os.listdir(d) if f.startswith(stem + "_")] == []


def plan_counts(n, plans, sol):
    for k in X.LISTS:
        f = plans[k]["flags"]
        cut = (f & _abi.AASM_CUT_IS_CUT) != 0
        ok = cut & ((f & _abi.AASM_CUT_ERRORS) == 0)
        n["elements"] += len(f); n["cut"] += int(cut.sum())
        n["irregular"] += int((ok & ((f & _abi.AASM_CUT_IRREGULAR) != 0)).sum())
        n["both"] += int((ok & (plans[k]["head_keep"] > 0) & (plans[k]["tail_keep"] > 0)).sum())
        n["empty"] += int((ok & (plans[k]["keep_lo"] == plans[k]["keep_hi"])).sum())
    n["alt"] += len(sol["alt"]); n["all"] += len(sol["all"])


def one_run(T, emc, emr, text, K, nsl, d, stem, n):
    api = T.api()
    exp = F.expected(T, text, K, nsl)
    host, dev = api.Paf.parse(text), api.Paf.parse(text, device_ranges=True)
    assert T.diff_outputs(exp.sol, T.emul_solve(host.batch(), K, nsl)) == []
    assert T.diff_outputs(exp.sol, emul_k0_solve(T, dev.view(), K, nsl)) == []
    rc, msg, epaf, eview = XR.emul_parse(emr, text)
    assert rc == 0, msg
    assert XR.diff_views(XR.view_arrays(dev.view()), eview) == [] and epaf.to_text() == dev.to_text()
    plans = X.emul_plans(emc, dev.view(), exp.sol)
    plan_flags_equal_verdict(plans, exp)
    bo, keep = X.pack_out(exp.sol)
    n["rejected_elements"] += sum(1 for k in X.LISTS for v in exp.verdict[k] if v)
    if exp.kind == "err":
        assert set(v for k in X.LISTS for v in exp.verdict[k]) == {0, 0x40}
        writers_fail_cleanly(api, dev, bo, plans, exp, d, stem)
        with pytest.raises(api.AlignasmError) as e:
            X.write_three(host, bo, d, stem + "_host")
        assert e.value.code == _abi.AASM_E_PARSE and exp.message in str(e.value)
        n["rejected"] += 1
        return
    n["accepted"] += 1
    want = list(exp.files)
    assert X.write_three(host, bo, d, stem + "_h") == want
    assert X.write_three(dev, bo, d, stem + "_d") == want
    assert X.write_three(dev, bo, d, stem + "_p", cuts=plans) == want
    paths = [os.path.join(str(d), stem + "_e" + s) for s in (".aln.paf", ".aln.alt.paf", ".aln.all.paf")]
    epaf.write_outputs(bo, *paths)                                   # the walking writer on the emulated reader's container
    assert [open(p, "rb").read() for p in paths] == want
    va = X.view_arrays(dev.view())
    hc = X.check_against_host(T, va, exp.sol, plans)
    assert hc["errors"] == 0
    plan_counts(n, plans, exp.sol)


def corpus(T, emc, emr, text_of, tmp_path):
    n = dict.fromkeys(("elements", "cut", "irregular", "both", "empty", "alt", "all", "accepted", "rejected", "rejected_elements"), 0)
    for i in range(N_TEXTS):
        for K, nsl in F.RUNS:
            try:
                one_run(T, emc, emr, text_of(i), K, nsl, tmp_path, "t%d_%d" % (i, K), n)
            except AssertionError as e:
                p = tmp_path / ("text_%d.paf" % i)
                p.write_bytes(text_of(i))
                raise AssertionError("text %d of seed %d, K = %d, nsl = %s (written to %s): %s" % (i, F.SEED, K, nsl, p, e)) from e
    return n


def test_shaped_texts(T, emc, emr, tmp_path):
    """72 runs.  The oracle accepts every one: 3 674 output elements, 2 625 of them cut, 492 alt and 316 .all elements; among the
    plans (checked against the oracle's rows first) 532 IRREGULAR, 179 with head and tail both shortened, 95 that keep no whole
    operation."""
    n = corpus(T, emc, emr, F.shaped_text, tmp_path)
    print(n)
    assert n["rejected"] == 0 and n["accepted"] == 2 * N_TEXTS
    assert n["cut"] >= 0.4 * n["elements"] and n["alt"] > 0 and n["all"] > 0, n
    assert n["irregular"] >= 50 and n["both"] >= 50 and n["empty"] >= 50, n


def test_unshaped_texts(T, emc, emr, tmp_path):
    """72 runs: in four records of ten (text_fuzz.SHAPED_SHARE says why not in all) any operation may come first or last, and a
    record that starts or ends with a deletion and is clipped at its other end keeps a reference coordinate the edited tag does
    not reach - the reference's own throw at paf_data.cpp:209-218.  The oracle rejects 35 runs (71 elements, all 'Edited cs tag
    does not match edited PAF coordinates') and accepts 37."""
    n = corpus(T, emc, emr, F.unshaped_text, tmp_path)
    print(n)
    assert n["rejected"] >= N_TEXTS // 2 and n["accepted"] >= N_TEXTS // 2 and n["rejected_elements"] >= 30, n


def test_many_contigs_text_is_what_the_gpu_tier_expects(T):
    """The two-contigs-per-wave shape: 2 700 contigs, every one accepted by the oracle, thousands of cut rows."""
    text = F.many_contigs_text(7, 1)
    exp = F.expected(T, text, 3, True)
    assert exp.kind == "ok" and exp.sol["n_contigs"] == 2700 and len(exp.sol["alt"]) > 0
    assert np.count_nonzero(exp.sol["status"]) == 0
