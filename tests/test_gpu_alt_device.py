"""GPU tier of the --alt merge on the device: DeviceBatch.merge_alt (aasm_paf_merge_alt_device, kernels aasm_alt_* behind the
reader's own) on every case of tests/alt_cases.py against the host route, array by array; the reader's hooks on a text of many
rows; both poison bytes; merged batch -> solve -> device writer against the host route's files and the golden ones; declined texts
leave the source batch as it was; a malformed tag in an alt row surfaces in the solve."""
import os

import pytest

import alt_cases as AC
import alt_testlib as XA
import cuts_testlib as XC
import poison_testlib as P
import read_cols_testlib as XR
import read_testlib as X
from alignasm_amd import _abi
from test_alt_device_cpu import HOOKS, _names
from test_golden import SUFFIXES

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "files")
K = 64


@pytest.fixture(scope="module")
def merging(T):
    """name -> (case, the host route's merged arrays): made once, shared by the plain, hooked and poisoned runs."""
    api = T.api()
    made = {}
    for case in AC.merging_cases(api) + [AC.big_case(api)]:
        before, want = XA.host_route(api, XA.uploaded_cols(api), case)
        assert case["meant"](before, want), case["name"]
        made[case["name"]] = (case, want)
    return made


@pytest.fixture(scope="module")
def declined(T):
    api = T.api()
    return {c["name"]: (c, XA.expected_decline(api, XA.uploaded_cols(api), c)) for c in AC.declined_cases(api)}


def _arrays(api, db):
    fetch = X.hip_fetcher(api)
    return {"view": X.view_arrays(db.dev_view, fetch), "cols": XR.cols_arrays(db.row_cols(), db.n_contigs, db.n_records, fetch)}


def _source(api, case, uploaded=False):
    """The main file resident with its row columns: read by the device reader, or uploaded from the host reader's container."""
    if uploaded:
        return api.DeviceBatch(api.Paf.parse(case["main"], device_ranges=True))
    return api.Paf.parse_device(case["main"], container=False)[1]


def _merge_and_check(api, case, want, flags=0, uploaded=False):
    src = _source(api, case, uploaded)
    before = _arrays(api, src)
    merges, verdicts = api.debug_counter("alt_device_merges"), api.debug_counter("alt_host_verdicts")
    db = P.guarded(api, src.merge_alt, case["alt"], case["baseline"], _flags=flags)
    assert (api.debug_counter("alt_device_merges"), api.debug_counter("alt_host_verdicts")) == (merges + 1, verdicts)
    assert XA.diff(want, _arrays(api, db)) == []
    assert XA.diff(before, _arrays(api, src)) == []                  # (the source batch is read only)
    db.close(); src.close()


@pytest.mark.parametrize("name", _names(AC.merging_cases))
def test_device_merge_equals_the_host_route(T, merging, name):
    case, want = merging[name]
    _merge_and_check(T.api(), case, want)
    _merge_and_check(T.api(), case, want, flags=HOOKS["weak_few"], uploaded=True)


@pytest.mark.parametrize("hook", ["none"] + sorted(HOOKS))
def test_hooks_on_many_rows(T, merging, hook):
    case, want = merging["big"]
    _merge_and_check(T.api(), case, want, flags=HOOKS.get(hook, 0))


@pytest.mark.parametrize("byte", P.BYTES, ids=P.BYTE_IDS)
@pytest.mark.parametrize("name", _names(AC.merging_cases) + ["big"])
def test_device_merge_with_poisoned_memory(T, merging, name, byte):
    case, want = merging[name]
    api = T.api()
    with P.poisoned(api, byte):
        _merge_and_check(api, case, want)


def _host_files(api, case, d, stem):
    paf = api.Paf.parse(case["main"])
    paf.merge_alt(case["alt"], case["baseline"])
    bo = api.solve_batch_raw(paf.view(), _abi.make_opts(K, False, 0, False, False))
    try:
        return XC.write_three(paf, bo, d, stem)
    finally:
        api.free_out(bo)


@pytest.mark.parametrize("name", ["tiny_0.5", "interleaved_runs"])
def test_merged_batch_solves_and_writes_the_host_routes_files(T, merging, tmp_path, name):
    api = T.api()
    case, _ = merging[name]
    want = _host_files(api, case, tmp_path, "h")
    assert len(want[0]) > 0
    src = _source(api, case)
    db = src.merge_alt(case["alt"], case["baseline"])
    res = db.solve(max_paths=K)
    paths = [str(tmp_path / ("d" + s)) for s in SUFFIXES]
    db.write_outputs(res, *paths)
    assert [open(p, "rb").read() for p in paths] == want
    d = res.to_torch(cuts=db, rows=True)
    assert "main_cut" in d
    if name == "tiny_0.5":
        assert want == [open(os.path.join(G, "alt", "tiny" + s), "rb").read() for s in SUFFIXES]
    res.close(); db.close(); src.close()


@pytest.mark.parametrize("name", _names(AC.declined_cases))
def test_declined_texts_leave_the_source_batch_solving_as_before(T, declined, name):
    api = T.api()
    case, (code, message) = declined[name]
    src = _source(api, case)
    before = _arrays(api, src)
    merges, verdicts = api.debug_counter("alt_device_merges"), api.debug_counter("alt_host_verdicts")
    with pytest.raises(api.AlignasmError) as got:
        src.merge_alt(case["alt"], case["baseline"])
    assert (got.value.code, str(got.value).split(": ", 1)[1]) == (code, message)
    assert (api.debug_counter("alt_device_merges"), api.debug_counter("alt_host_verdicts")) == (merges, verdicts + 1)
    for byte in P.BYTES:                                             # the verdict does not hang on what fresh working memory holds
        with P.poisoned(api, byte):
            with pytest.raises(api.AlignasmError) as again:
                P.guarded(api, src.merge_alt, case["alt"], case["baseline"], _flags=HOOKS["weak_few"])
        assert (again.value.code, str(again.value)) == (got.value.code, str(got.value))
    assert XA.diff(before, _arrays(api, src)) == []
    if name in ("zeroed_group", "two_faults_first_is_named"):
        res = src.solve(max_paths=K)
        out = res.fetch()                                            # (before the next solve on the device, which invalidates the result)
        res.close()
        assert T.diff_outputs(api.solve_batch(api.Paf.parse(case["main"]), max_paths=K), out, stats=False) == []
    src.close()


def test_a_malformed_alt_tag_merges_and_fails_in_the_solve(T):
    api = T.api()
    case = AC.bad_tag_case(api)
    src = _source(api, case)
    db = src.merge_alt(case["alt"], case["baseline"])
    assert db.n_records == src.n_records + 1
    with pytest.raises(api.AlignasmError) as got:
        db.solve(max_paths=K)
    assert got.value.code == _abi.AASM_E_PARSE
    db.close(); src.close()


def test_a_batch_without_row_columns_or_paf_is_refused(T):
    api = T.api()
    hb = api.Paf.parse(AC.main_text(api), device_ranges=True).batch()
    src = api.DeviceBatch(hb)
    with pytest.raises(api.AlignasmError) as got:
        src.merge_alt(b"", 0.5)
    assert got.value.code == _abi.AASM_E_INVAL
    src.close()
