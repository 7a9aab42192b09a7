"""Differential fuzzing of the device reader, GPU tier: aasm_paf_parse_device on the MI355X against the host reader on the random
texts of tests/read_fuzz.py (the first of the CPU tier's corpus): what only the device can get wrong - wave scans, racing atomics
in the reference-name table, the order of the slow list, sixteen lanes per tag, sixteen-byte loads.  A read costs dozens of
allocations and waits (DESIGN.md section 7 has the time per read), hence the counts."""
import pytest

import read_fuzz as F
import read_testlib as X
from alignasm_amd import _abi
from test_read_fuzz_cpu import host_verdict, run

pytestmark = pytest.mark.gpu
N_STRUCTURED, N_MUTANTS = 150, 300


def check_device(api, fetch, verdict, text, flags):
    code, want, want_text = verdict
    before = api.debug_counter("read_host_fallbacks")
    if code != 0:
        with pytest.raises(api.AlignasmError) as ei:
            api.Paf.parse_device(text, _flags=flags)
        assert ei.value.code == code != _abi.AASM_E_INTERNAL and str(ei.value).split(": ", 1)[1] == want
        assert api.debug_counter("read_host_fallbacks") == before + 1
        return
    up = api.DeviceBatch(api.Paf.parse(text, device_ranges=True))   # what aasm_upload_batch gives for the host-read container
    paf, db = api.Paf.parse_device(text, _flags=flags)
    try:
        assert api.debug_counter("read_host_fallbacks") == before and api.debug_counter("read_slow_rows") == F.expected_slow(text)
        got_dev = X.view_arrays(db.dev_view, fetch)
        assert X.diff_views(want, X.view_arrays(paf.view())) == [] and paf.to_text() == want_text
        assert X.diff_views(want, got_dev) == []
        assert X.diff_views(X.view_arrays(up.dev_view, fetch), got_dev) == []
    finally:
        db.close(); up.close(); paf.close()


def test_structured_texts_on_the_device(T, tmp_path):
    """A third under the weak hash, a third with every grid capped at 3 blocks."""
    api = T.api()
    fetch = X.hip_fetcher(api)
    for i in range(N_STRUCTURED):
        text, _ = F.structured_text(i)
        verdict = host_verdict(api, text)
        flags = (_abi.AASM_READ_H_WEAK_HASH, _abi.AASM_READ_H_FEW_BLOCKS, 0)[i % 3]

        def check():
            assert verdict[0] == 0, verdict[1]
            check_device(api, fetch, verdict, text, flags)
        run("structured", i, text, tmp_path, check)


def test_mutants_on_the_device(T, tmp_path):
    api = T.api()
    fetch = X.hip_fetcher(api)
    n_accepted = 0
    for i in range(N_MUTANTS):
        text = F.mutant_text(i)
        verdict = host_verdict(api, text)
        n_accepted += verdict[0] == 0
        run("mutant", i, text, tmp_path, lambda: check_device(api, fetch, verdict, text, 0))
    assert 0.15 * N_MUTANTS <= n_accepted <= 0.85 * N_MUTANTS       # (the host reader's verdicts: both halves of the contract ran)
