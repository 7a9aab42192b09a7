"""`alignasm --device-reader --device-writer --device-alt -a ALT`: route 1 with the alt file merged on the device
(alignasm_amd/csrc/alignasm_main.cpp).  GPU tier: the golden alt files without a container; alt files the device declines or whose
tags the solve rejects end as the plain command does.  CPU tier: without a device the new cells end where their siblings do, and
the flag's two usage errors."""
import os
import subprocess

import pytest

import alt_cases as AC
from test_cli_routes import H, NO_DEVICE, R, W, _exe, _golden, _run, inputs, no_device  # noqa: F401 (fixtures)
from test_golden import SUFFIXES

A = "--device-alt"


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------
def test_without_a_device_the_new_cells_end_where_their_siblings_do(T, no_device, tmp_path, inputs):
    for name in ("tiny.paf", "empty.paf", "no_cs.paf"):
        for flags in ([R, W, A, "-a", tmp_path / "tiny_alt.paf"], [R, W, A], [R, W, A, "-a", tmp_path / "empty.paf"]):
            assert _run(T, [tmp_path / name] + flags) == NO_DEVICE, (name, flags)
            assert sorted(p.name for p in tmp_path.iterdir()) == inputs, (name, flags)


def test_usage_errors_of_the_flag(T, no_device, tmp_path, inputs):
    p = str(tmp_path / "tiny.paf")
    cells = [
        ([p, A, H], "--device-alt: not with --host-ranges\nUsage: alignasm"),
        ([p, A, "--gpus", "2"], "--device-alt: not with --gpus above 1\nUsage: alignasm"),
        ([p, R, W, A, H, "--gpus", "2"], "--device-reader: not with --host-ranges\n--device-writer: not with --host-ranges\n--device-alt: not with --host-ranges\n"
                                         "--device-writer: not with --gpus above 1\n--device-alt: not with --gpus above 1\nUsage: alignasm"),
    ]
    usage = _run(T, ["--help"])
    assert usage[0] == 0 and "[--device-alt]" in usage[1] and "\n  --device-alt " in usage[1]
    for args, head in cells:
        code, out, err = _run(T, args)
        assert code == 1 and out == "" and err == head + usage[1][len("Usage: alignasm"):], (args, err)
        assert sorted(q.name for q in tmp_path.iterdir()) == inputs, args


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------
def _split(err):
    lines = err.split("\n")
    timing = [ln for ln in lines if ln.startswith("alignasm timing:")]
    return timing, [ln for ln in lines if ln not in timing]


def _files(d, stem, remove=True):
    paths = [d / (stem + s) for s in SUFFIXES]
    got = [p.read_bytes() if p.exists() else None for p in paths]
    for p in paths:
        if remove and p.exists():
            p.unlink()
    return got


@pytest.mark.gpu
def test_the_golden_alt_files_are_written_without_a_container(T, tmp_path):
    for name in ("tiny.paf", "tiny_alt.paf"):
        (tmp_path / name).write_bytes(_golden(name))
    args = [tmp_path / "tiny.paf", "-a", tmp_path / "tiny_alt.paf", "--timing"]
    plain = _run(T, args)
    plain_files = _files(tmp_path, "tiny")
    code, out, err = _run(T, args + [R, W, A])
    timing, rest = _split(err)
    print(code, repr(out), err, flush=True)
    assert code == 0 and out == plain[1] and rest == _split(plain[2])[1] == [""]
    assert len(timing) == 1 and timing[0].endswith(" container 0")
    files = _files(tmp_path, "tiny")
    assert files == [_golden("alt", "tiny" + s) for s in SUFFIXES] == plain_files
    # without --device-alt the same command line builds the container, as before
    code, out, err = _run(T, args + [R, W])
    assert code == 0 and _split(err)[0][0].endswith(" container 1") and _files(tmp_path, "tiny") == files
    # the flag alone changes nothing, nor does it with an empty alt file (which is no --alt: route 1 as before)
    (tmp_path / "none_alt.paf").write_bytes(b"")
    code, out, err = _run(T, [tmp_path / "tiny.paf", "-a", tmp_path / "none_alt.paf", "--timing", R, W, A])
    assert code == 0 and _split(err)[0][0].endswith(" container 0") and _files(tmp_path, "tiny") == [_golden("tiny" + s) for s in SUFFIXES]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["zeroed_group", "start_with_a_sign", "name_x_9", "no_cs_tag", "bad_tag", "interleaved_runs"])
def test_alt_files_end_as_the_plain_command_does(T, tmp_path, kind):
    """Declined by the device (the host merges it, or names its fault), a tag only the solve finds, and a text that merges."""
    api = T.api()
    cases = {c["name"]: c for c in AC.declined_cases(api) + [AC.bad_tag_case(api)] + [c for c in AC.merging_cases(api) if c["name"] == "interleaved_runs"]}
    case = cases[kind]
    (tmp_path / "m.paf").write_bytes(case["main"])
    (tmp_path / "a.paf").write_bytes(case["alt"])
    args = [tmp_path / "m.paf", "-a", tmp_path / "a.paf", "--max-paths", "64", "--timing"]
    runs = []
    for extra in ([], [R, W, A]):
        code, out, err = _run(T, args + extra)
        timing, rest = _split(err)
        print(kind, extra, code, repr(out), err, flush=True)
        runs.append((code, out, rest, _files(tmp_path, "m")))
        if code == 0:
            assert timing[0].endswith(" container %d" % (0 if extra and kind == "interleaved_runs" else 1))
    assert runs[1] == runs[0]
    # (the host merges the zeroed group, but its stand-in record has no tag: the plain command's solve rejects it, exit 1)
    assert (runs[0][0] == 0) == (kind in ("start_with_a_sign", "interleaved_runs")) and (None in runs[0][3]) == (runs[0][0] != 0)
