"""Differential fuzzing of the device reader, CPU tier: the 1-lane emulation (tests/host_emul/read_emul.cpp) against the host reader on the
random texts of tests/read_fuzz.py.  For any byte string both take the text and give the same container and batch, or both refuse
it with the same code and message; AASM_E_INTERNAL never appears.  What the corpus must contain is asserted on the host reader's
verdicts alone, so that a change to the generator cannot turn the run into all-accepts or all-rejects unnoticed."""
import collections

import pytest

import read_fuzz as F
import read_testlib as X
from alignasm_amd import _abi

N_STRUCTURED, N_MUTANTS = 1500, 4500                                 # about 20 s with the emulation's build
KINDS = ("fewer than 12 columns", "non-numeric field", "Missing cs:Z tag")


@pytest.fixture(scope="module")
def emr():
    return X.build_emul()


def host_verdict(api, text):
    """The yardstick -> (0, arrays, to_text()) or (code, message, None)."""
    try:
        paf = api.Paf.parse(text, device_ranges=True)
    except api.AlignasmError as e:
        return e.code, str(e).split(": ", 1)[1], None
    return 0, X.view_arrays(paf.view()), paf.to_text()


def check_emulated(lib, verdict, text, modes):
    """One text through the emulation in every mode (flags, max_blocks) against the host reader's verdict."""
    code, want, want_text = verdict
    for flags, max_blocks in modes:
        before = lib.emr_counter(1)
        rc, msg, paf, view = X.emul_parse(lib, text, flags, max_blocks)
        assert rc != _abi.AASM_E_INTERNAL, msg
        if code == 0:
            assert rc == 0, msg
            assert X.diff_views(want, X.view_arrays(paf.view())) == [] and X.diff_views(want, view) == []
            assert paf.to_text() == want_text
            assert lib.emr_counter(0) == F.expected_slow(text) and lib.emr_counter(1) == before
        else:
            assert (rc, msg) == (code, want) and paf is None and view is None
            assert lib.emr_counter(1) == before + 1


def modes_of(i):
    """max_blocks 0 and 3 (the grid-stride loops); every tenth text under the weak hash as well."""
    hashes = (0, _abi.AASM_READ_H_WEAK_HASH) if i % 10 == 0 else (0,)
    return [(h, b) for h in hashes for b in (0, 3)]


def run(what, i, text, tmp_path, check):
    try:
        check()
    except AssertionError as e:
        path = tmp_path / ("%s_%d.paf" % (what, i))
        path.write_bytes(text)
        raise AssertionError("%s text %d of seed %d (written to %s): %s" % (what, i, F.SEED, path, e)) from e


def test_structured_texts(T, emr, tmp_path):
    api = T.api()
    n_strict = n_edge = 0
    for i in range(N_STRUCTURED):
        text, strict = F.structured_text(i)
        verdict = host_verdict(api, text)

        def check():
            assert verdict[0] == 0, verdict[1]                       # (the generator makes valid texts)
            check_emulated(emr, verdict, text, modes_of(i))
            if strict:
                rc, msg, paf, _ = X.emul_parse(emr, text, want_view=False)
                assert rc == 0, msg
                X.check_against_oracle(T, text, X.view_arrays(paf.view()), paf.to_text())
        run("structured", i, text, tmp_path, check)
        n_strict += strict
        n_edge += F.row_start_near_edge(text)
    assert n_strict >= N_STRUCTURED // 4 and n_edge >= 20


@pytest.fixture(scope="module")
def mutants(T):
    """(text, the host reader's verdict) of every mutant."""
    api = T.api()
    out = []
    for i in range(N_MUTANTS):
        text = F.mutant_text(i)
        out.append((text, host_verdict(api, text)))
    return out


def test_the_mutants_are_a_mix(mutants):
    """Conditions on the corpus, from the host reader alone."""
    accepted = [t for t, v in mutants if v[0] == 0]
    messages = [v[1] for _, v in mutants if v[0] != 0]
    assert len(accepted) >= 0.15 * N_MUTANTS and len(messages) >= 0.15 * N_MUTANTS
    assert all(v[0] in (0, _abi.AASM_E_PARSE) for _, v in mutants)
    kinds = collections.Counter(k for m in messages for k in KINDS if k in m)
    assert all(kinds[k] >= 20 for k in KINDS), kinds
    assert sum(F.expected_slow(t) > 0 for t in accepted) >= 20
    assert sum(F.row_start_near_edge(t) for t, _ in mutants) >= 20


def test_mutants(emr, mutants, tmp_path):
    for i, (text, verdict) in enumerate(mutants):
        run("mutant", i, text, tmp_path, lambda: check_emulated(emr, verdict, text, modes_of(i)))
