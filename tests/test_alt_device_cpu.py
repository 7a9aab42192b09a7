"""CPU tier of the --alt merge on the device (alignasm_amd/csrc/aasm_alt.h): alt_merge_run in the 1-lane host emulation on every
case of tests/alt_cases.py against the host route - aasm_paf_parse_mem_opts(main, AASM_READ_DEVICE_RANGES) ->
aasm_paf_merge_alt_mem -> aasm_paf_batch + the container's row columns - array by array, and against the I/O oracle's own merge;
the declined texts' code and message; the reader's two test hooks on a text of many rows; the same cases through the program built
with the host address sanitizer."""
import subprocess

import pytest

import alt_cases as AC
import alt_testlib as XA
from alignasm_amd import _abi

HOOKS = {"weak": _abi.AASM_READ_H_WEAK_HASH, "few": _abi.AASM_READ_H_FEW_BLOCKS, "weak_few": _abi.AASM_READ_H_WEAK_HASH | _abi.AASM_READ_H_FEW_BLOCKS}


@pytest.fixture(scope="module")
def built():
    return XA.build_emul(san=True)


@pytest.fixture(scope="module")
def lib(built):
    return built[0]


@pytest.fixture(scope="module")
def merging(T, lib):
    """name -> (case, main arrays, the host route's merged arrays): each text does, on the host, what it is meant to do."""
    api = T.api()
    made = {}
    for case in AC.merging_cases(api) + [AC.big_case(api)]:
        before, want = XA.host_route(api, XA.emul_cols(lib), case)
        assert case["meant"](before, want), case["name"]
        made[case["name"]] = (case, before, want)
    return made


@pytest.fixture(scope="module")
def declined(T, lib):
    api = T.api()
    return {c["name"]: (c, XA.expected_decline(api, XA.emul_cols(lib), c)) for c in AC.declined_cases(api)}


def _names(fn):
    import aasm_testlib as T
    return [c["name"] for c in fn(T.api())]


@pytest.mark.parametrize("name", _names(AC.merging_cases))
def test_emulated_merge_equals_the_host_route(T, lib, merging, name):
    case, _, want = merging[name]
    merges = lib.emalt_counter(1)
    for cap in (0, 3):
        rc, msg, got = XA.emul_merge(lib, T.api(), case, max_blocks=cap)
        assert rc == 0, msg
        assert XA.diff(want, got) == []
    assert lib.emalt_counter(1) == merges + 2
    if case["oracle"]:
        XA.check_against_oracle(T, case, got)


@pytest.mark.parametrize("name", _names(AC.declined_cases))
def test_declined_texts_give_the_code_and_the_message(T, lib, declined, name):
    """emalt_merge itself returns AASM_E_INTERNAL where a call has written into its input arrays."""
    case, (code, message) = declined[name]
    verdicts = lib.emalt_counter(0)
    for flags in (0, HOOKS["weak_few"]):
        rc, msg, got = XA.emul_merge(lib, T.api(), case, flags=flags)
        assert (rc, msg, got) == (code, message, None)
    assert code == -7 and lib.emalt_counter(0) == verdicts + 2


@pytest.mark.parametrize("hook", sorted(HOOKS))
def test_hooks_on_many_rows(T, lib, merging, hook):
    """>= 1 100 alt rows in more than two reader tiles: colliding slots in both name tables, grids of 3 blocks."""
    case, _, want = merging["big"]
    rc, msg, got = XA.emul_merge(lib, T.api(), case, flags=HOOKS[hook])
    assert rc == 0, msg
    assert XA.diff(want, got) == []
    if hook == "weak_few":
        XA.check_against_oracle(T, case, got)


def test_a_malformed_tag_merges_on_the_device_and_not_on_the_host(T, lib):
    """The host merge validates an alt row's tag; the device leaves that to the solve, as with AASM_READ_DEVICE_RANGES."""
    api = T.api()
    case = AC.bad_tag_case(api)
    assert XA.host_verdict(api, XA.emul_cols(lib), case)[0] == -7
    rc, msg, got = XA.emul_merge(lib, api, case)
    assert rc == 0 and got["view"]["n_records"] == 33 and got["cols"]["cord_type"][8] == 1


def test_the_sanitizer_program_runs_every_case(T, built, merging, declined, tmp_path):
    """alt_emul_san: the same bodies with the host address sanitizer and exact-size blocks, every hook, grids free and capped."""
    san = built[1]
    args, want = [], []
    files = {}

    def path(data):
        if data not in files:
            files[data] = str(tmp_path / f"f{len(files)}.paf")
            open(files[data], "wb").write(data)
        return files[data]
    for name, (case, _, merged) in merging.items():
        if name == "big":
            continue
        args += [path(case["main"]), path(case["alt"]), repr(case["baseline"])]
        want += [(0, int(merged["view"]["n_records"]), int(merged["cols"]["n_chr"]))] * 8
    for name, (case, (code, _)) in declined.items():
        args += [path(case["main"]), path(case["alt"]), repr(case["baseline"])]
        want += [(code, -1, -1)] * 8
    run = subprocess.run([san] + args, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [tuple(int(x) for x in ln.split()[2:5]) for ln in run.stdout.splitlines()]
    assert got == want
