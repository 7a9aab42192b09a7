"""The route ladder of the `alignasm` command line (alignasm_amd/csrc/alignasm_main.cpp, the table in its header comment).
CPU tier: without a device every route ends at a fixed place, so (file, flags) -> (exit code, stdout, stderr) is pinned cell by cell,
with the usage errors.  GPU tier: none / --device-reader / --device-writer / both must agree in exit code, stdout, stderr (less the
--timing line) and the three files, on inputs that between them take every route and every fallback; golden bytes where they exist."""
import os
import re
import subprocess

import pytest

import read_cases as RC
import text_fuzz as F
from test_golden import SUFFIXES

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "files")
R, W, H = "--device-reader", "--device-writer", "--host-ranges"


def _exe(T):
    return os.path.join(T.ROOT, "alignasm_amd", "alignasm")


def _golden(*parts):
    return open(os.path.join(G, *parts), "rb").read()


def _run(T, args):
    r = subprocess.run([_exe(T)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


# ---- CPU tier ---------------------------------------------------------------------------------------------------------------------
NO_DEVICE = (2, "", "alignasm: solver failed (-2): no HIP device available (this library has no CPU fallback)\n")
TINY_READ = (2, "File read complete\nAnalyze PAF 3 data in parallel\n", NO_DEVICE[2])     # the host reader got through; the solve did not
EMPTY = (1, "", "empty PAF\n")
NO_CS = (1, "", "Missing cs:Z tag in PAF record for query 'ctgN'\n")
FLAG_SETS = {"none": [], "reader": [R], "writer": [W], "both": [R, W], "host_ranges": [H], "both_alt": [R, W, "-a", "tiny_alt.paf"]}
# with --device-reader the first thing any route does is open the device; without it the host reader reads (and judges) the file first
NO_DEVICE_TABLE = {
    "tiny.paf": {"none": TINY_READ, "reader": NO_DEVICE, "writer": TINY_READ, "both": NO_DEVICE, "host_ranges": TINY_READ, "both_alt": NO_DEVICE},
    "empty.paf": {"none": EMPTY, "reader": NO_DEVICE, "writer": EMPTY, "both": NO_DEVICE, "host_ranges": EMPTY, "both_alt": NO_DEVICE},
    "no_cs.paf": {"none": NO_CS, "reader": NO_DEVICE, "writer": NO_CS, "both": NO_DEVICE, "host_ranges": NO_CS, "both_alt": NO_DEVICE},
}


@pytest.fixture
def no_device(T):
    if T.api().device_count() > 0:
        pytest.skip("the table is what the command does on a machine without a device")


@pytest.fixture
def inputs(tmp_path):
    for name in ("tiny.paf", "tiny_alt.paf"):
        (tmp_path / name).write_bytes(_golden(name))
    (tmp_path / "empty.paf").write_bytes(b"")
    (tmp_path / "no_cs.paf").write_bytes(RC.row(b"ctgA") + RC.row(b"ctgN", tags=[b"tp:A:P"]) + RC.row(b"ctgA", qs=500))
    return sorted(p.name for p in tmp_path.iterdir())


@pytest.mark.parametrize("name", sorted(NO_DEVICE_TABLE))
def test_without_a_device_every_cell_ends_where_the_table_says(T, no_device, tmp_path, inputs, name):
    for key, flags in FLAG_SETS.items():
        flags = [str(tmp_path / f) if f.endswith(".paf") else f for f in flags]
        assert _run(T, [tmp_path / name] + flags) == NO_DEVICE_TABLE[name][key], (name, key)
        assert sorted(p.name for p in tmp_path.iterdir()) == inputs, (name, key)


def test_usage_errors_exit_1_with_the_usage_on_stderr(T, no_device, tmp_path, inputs):
    p = str(tmp_path / "tiny.paf")
    cells = [
        ([p, "--no-such-flag"], "Unknown argument: --no-such-flag\nUsage: alignasm"),
        ([p, "--max-paths"], "--max-paths: missing value\nUsage: alignasm"),
        ([p, "-a"], "--alt: missing value\nUsage: alignasm"),
        ([p, p], "Maximum number of positional arguments exceeded\nUsage: alignasm"),
        ([], "Usage: alignasm"),
        ([tmp_path / "tiny.txt"], 'Wrong PAF file : "%s"Usage: alignasm' % (tmp_path / "tiny.txt")),
        ([p, "-a", tmp_path / "alt.txt"], 'Wrong PAF file : "%s"Usage: alignasm' % (tmp_path / "alt.txt")),
        ([p, R, H], "--device-reader: not with --host-ranges\nUsage: alignasm"),
        ([p, W, H], "--device-writer: not with --host-ranges\nUsage: alignasm"),
        ([p, W, "--gpus", "2"], "--device-writer: not with --gpus above 1\nUsage: alignasm"),
        ([p, R, W, H, "--gpus", "2"], "--device-reader: not with --host-ranges\n--device-writer: not with --host-ranges\n"
                                      "--device-writer: not with --gpus above 1\nUsage: alignasm"),
    ]
    usage = _run(T, ["--help"])
    assert usage[0] == 0 and usage[1].startswith("Usage: alignasm") and usage[2] == ""
    assert _run(T, ["--version"]) == (0, "0.1.0\n", "")
    for args, head in cells:
        code, out, err = _run(T, args)
        assert code == 1 and out == "" and err == head + usage[1][len("Usage: alignasm"):], (args, err)
        assert sorted(q.name for q in tmp_path.iterdir()) == inputs, args


# ---- GPU tier ---------------------------------------------------------------------------------------------------------------------
def _tiny(T, d):
    (d / "tiny.paf").write_bytes(_golden("tiny.paf"))
    return d / "tiny.paf", ["--timing"], ("",)


def _dense(T, d):
    (d / "dense.paf").write_bytes(_golden("dense.paf"))
    return d / "dense.paf", [], ("dense",)


def _tiny_alt(T, d):
    (d / "tiny_alt.paf").write_bytes(_golden("tiny_alt.paf"))
    return _tiny(T, d)[0], ["--timing", "-a", d / "tiny_alt.paf"], ("alt",)


def _tiny_empty_alt(T, d):                         # an empty alt file is no --alt: the plain bytes, and both flags build no container
    (d / "none_alt.paf").write_bytes(b"")
    return _tiny(T, d)[0], ["--timing", "-a", d / "none_alt.paf"], ("",)


def _streaming_shape(T, d):                        # plain: contig ranges; --device-reader: resident solve; writer flags: one piece on the device
    T.api().Paf.synth(120, 600, 3, dup_every=7).save(str(d / "s.paf"))
    return d / "s.paf", ["--max-paths", "16"], None


def _text(name, make):
    def build(T, d):
        (d / (name + ".paf")).write_bytes(make(T))
        return d / (name + ".paf"), [], None
    build.__name__ = name
    return build


GPU_INPUTS = [
    _tiny, _dense, _tiny_alt, _tiny_empty_alt, _streaming_shape,
    _text("empty", lambda T: b""),
    _text("later_kind_first", lambda T: dict(RC.error_cases())["later_kind_first"]),
    _text("bad_tag_only", lambda T: RC.bad_tag_only()),
    _text("unshaped_rejected", lambda T: next(F.unshaped_text(i) for i in range(8) if F.expected(T, F.unshaped_text(i), 10000, False).kind == "err")),
]
GOOD = (_tiny, _dense, _tiny_alt, _tiny_empty_alt, _streaming_shape)


@pytest.mark.gpu
@pytest.mark.parametrize("build", GPU_INPUTS, ids=lambda b: b.__name__.lstrip("_"))
def test_the_four_flag_sets_agree(T, tmp_path, build):
    path, flags, golden = build(T, tmp_path)
    outs = [tmp_path / (path.name[:-4] + s) for s in SUFFIXES]
    runs = []
    for extra in ([], [R], [W], [R, W]):
        code, out, err = _run(T, [path] + flags + extra)
        lines = err.split("\n")
        timing = [ln for ln in lines if ln.startswith("alignasm timing:")]
        files = [p.read_bytes() if p.exists() else None for p in outs]
        for p in outs:
            if p.exists():
                p.unlink()
        print(path.name, flags[:1], extra, code, repr(out), lines, [f if f is None else len(f) for f in files], flush=True)
        if "--timing" in flags:
            no_container = extra == [R, W] and build in (_tiny, _tiny_empty_alt)
            assert len(timing) == 1 and timing[0].endswith(" container %d" % (0 if no_container else 1)), (extra, err)
        else:
            assert timing == []
        runs.append((code, out, [ln for ln in lines if ln not in timing], files))
    assert runs[1] == runs[0] and runs[2] == runs[0] and runs[3] == runs[0], [r[:3] for r in runs]
    if build in GOOD:
        assert runs[0][0] == 0 and runs[0][2] == [""] and None not in runs[0][3]
        assert re.fullmatch(r"File read complete\nAnalyze PAF \d+ data in parallel\nWrite output PAF file\n", runs[0][1])
    else:
        assert runs[0][0] != 0 and runs[0][3] == [None, None, None]          # (a row that cannot be re-cut fails in the writer: exit 3, nothing committed)
    if golden is not None:
        assert runs[0][3] == [_golden(*golden, path.name[:-4] + s) for s in SUFFIXES]
