"""GPU tier of the text fuzz (tests/text_fuzz.py): the adversarial texts through every route from PAF text to written rows on the
MI355X - host ranges, K0 on the card, the device reader with export and cut plans resident, the command line both ways - against
the oracle side alone (tests/text_fuzz.py, expected()).  The texts are sized by their count: six contigs per text is the shape."""
import os
import subprocess

import pytest

import cuts_testlib as X
import text_fuzz as F
from alignasm_amd import _abi

pytestmark = pytest.mark.gpu
FORMS = {"default": {}, "chain_none": {"chain": "none"}, "chain_all": {"chain": "all"}, "heap_waves_all": {"heap_waves": "all"},
         "sequential_select": {"sequential_select": True}}
N_SHAPED, N_UNSHAPED = 30, 24                                        # text i runs under form i % 5
SUFFIXES = (".aln.paf", ".aln.alt.paf", ".aln.all.paf")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("the GPU tier needs torch to see the device")
    return torch


def resident(T, torch, db, K, nsl, hooks):
    """solve -> export -> cut plans on a resident batch -> (fetched solution, raw result for the writers, exported arrays, plans)."""
    api = T.api()
    res = db.solve(max_paths=K, non_skip_linkable=nsl, **hooks)
    d = res.to_torch(cuts=db)
    torch.cuda.current_stream(db.device).synchronize()
    out = (res.fetch(), res.fetch_raw(), api.torch_to_numpy(d), api.cuts_to_numpy(d))
    res.close()
    return out


def routes(T, torch, text, K, nsl, hooks, d, stem, every=1):
    """One text through (a) host ranges, (b) K0 on the card, (c) the device reader -> (Expected, device plans of (c)).  Every
    `every`-th plan of each list goes against the host codec."""
    api = T.api()
    exp = F.expected(T, text, K, nsl)
    # (a) the host reader's match ranges
    host = api.Paf.parse(text)
    got_a = api.solve_batch(host, max_paths=K, non_skip_linkable=nsl, **hooks)
    assert T.diff_outputs(exp.sol, got_a) == [], "a"
    # (b) the tags uploaded, K0 on the card
    dev = api.Paf.parse(text, device_ranges=True)
    db = api.DeviceBatch(dev)
    got_b, bo_b, out_b, plans_b = resident(T, torch, db, K, nsl, hooks)
    db.close()
    assert T.diff_outputs(exp.sol, got_b) == [], "b"
    # (c) reader, K0, solve, export and cut plans, all resident
    paf_c, db_c = api.Paf.parse_device(text)
    got_c, bo_c, out_c, plans_c = resident(T, torch, db_c, K, nsl, hooks)
    db_c.close()
    try:
        assert T.diff_outputs(exp.sol, got_c) == [], "c"
        for k in X.LISTS:
            assert out_c[k].tobytes() == exp.sol[k].tobytes() and plans_c[k].tobytes() == plans_b[k].tobytes(), k
            assert [int(f) & _abi.AASM_CUT_ERRORS for f in plans_c[k]["flags"]] == exp.verdict[k], k
        if exp.kind == "ok":
            which = {k: range(0, len(out_c[k]), every) for k in X.LISTS}
            n = X.check_against_host(T, X.view_arrays(paf_c.view()), out_c, plans_c, which)
            assert n["errors"] == 0 and n["elements"] == sum(len(which[k]) for k in X.LISTS)
            want = list(exp.files)
            bo_a, keep = X.pack_out(got_a)
            assert X.write_three(host, bo_a, d, stem + "_a") == want, "a"
            assert X.write_three(dev, bo_b, d, stem + "_b") == want, "b"
            assert X.write_three(paf_c, bo_c, d, stem + "_c", cuts=plans_c) == want, "c"
        else:
            for what, cuts in (("walk", None), ("plan", plans_c)):
                with pytest.raises(api.AlignasmError) as e:
                    X.write_three(paf_c, bo_c, d, "%s_%s" % (stem, what), cuts=cuts)
                assert e.value.code == _abi.AASM_E_PARSE and exp.message in str(e.value), what
            assert [f for f in os.listdir(d) if f.startswith(stem + "_")] == []
    finally:
        api.free_out(bo_b); api.free_out(bo_c)
    return exp, plans_c


def run_texts(T, torch, text_of, numbers, hooks, tmp_path):
    kinds = {"ok": 0, "err": 0}
    for i in numbers:
        for K, nsl in F.RUNS:
            try:
                exp, _ = routes(T, torch, text_of(i), K, nsl, hooks, tmp_path, "t%d_%d" % (i, K))
            except AssertionError as e:
                p = tmp_path / ("text_%d.paf" % i)
                p.write_bytes(text_of(i))
                raise AssertionError("text %d of seed %d, K = %d, nsl = %s, %s (written to %s): %s" % (i, F.SEED, K, nsl, hooks, p, e)) from e
            kinds[exp.kind] += 1
    return kinds


@pytest.mark.parametrize("form", list(FORMS))
def test_shaped_texts_come_out_the_same_on_every_route(T, torch, tmp_path, form):
    """Solutions equal the solver oracle, files equal the oracle side's byte for byte, device plans equal the host codec on every
    element; a fifth of the texts under each launch form."""
    at = list(FORMS).index(form)
    kinds = run_texts(T, torch, F.shaped_text, range(at, N_SHAPED, len(FORMS)), FORMS[form], tmp_path)
    assert kinds == {"ok": 2 * len(range(at, N_SHAPED, len(FORMS))), "err": 0}


def test_unshaped_texts_carry_the_oracles_error_flags(T, torch, tmp_path):
    """Routes (b) and (c) give the oracle's solution; the device plans carry 0x40 on exactly the elements the reference's
    consistency throw rejects; both writers refuse such a file with the oracle's text and leave nothing behind.  Of the 48 runs
    the oracle rejects 23 and accepts 25."""
    kinds = run_texts(T, torch, F.unshaped_text, range(N_UNSHAPED), {}, tmp_path)
    assert kinds["err"] >= N_UNSHAPED // 2 and kinds["ok"] >= N_UNSHAPED // 2, kinds     # (a quarter of the runs each)


@pytest.mark.parametrize("case", [(7, 0, 10000, False), (8, 1, 3, True)], ids=["seed7_style0_k10000", "seed8_style1_k3_nsl"])
def test_many_contigs_texts(T, torch, tmp_path, case):
    """2 700 contigs: the sweeps run two contigs per wave.  Every 16th plan of each list against the host codec (every plan is
    in the written files, which are compared whole)."""
    seed, style, K, nsl = case
    exp, plans = routes(T, torch, F.many_contigs_text(seed, style), K, nsl, {}, tmp_path, "many", every=16)
    assert exp.kind == "ok" and exp.sol["n_contigs"] == 2700
    assert sum(int((plans[k]["flags"] & _abi.AASM_CUT_IS_CUT != 0).sum()) for k in X.LISTS) > 3000


def _cli(exe, path, flags, tmp_path):
    runs = []
    for extra in ([], ["--device-reader"]):
        r = subprocess.run([exe, str(path)] + flags + extra, capture_output=True, text=True, timeout=120)
        files = []
        for s in SUFFIXES:
            p = tmp_path / (path.name[:-4] + s)
            files.append(p.read_bytes() if p.exists() else None)
            if p.exists():
                p.unlink()
        runs.append((r.returncode, r.stderr, files))
    return runs


def test_command_line_both_ways(T, tmp_path):
    """`alignasm` with and without --device-reader on files joined from the texts (one process start is slow): shaped texts give
    the oracle side's files; a file with unshaped texts ends non-zero both ways with the same stderr, the oracle's text in it, and
    no output file."""
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    for name, first, (K, nsl) in (("s0", 0, F.RUNS[0]), ("s1", 10, F.RUNS[1])):
        text = F.joined([F.shaped_text(i) for i in range(first, first + 10)])
        exp = F.expected(T, text, K, nsl)
        assert exp.kind == "ok"
        path = tmp_path / (name + ".paf")
        path.write_bytes(text)
        runs = _cli(exe, path, ["--max-paths", str(K)] + (["--non_skip_linkable"] if nsl else []), tmp_path)
        assert runs[0][0] == 0 and runs[1][0] == 0, (runs[0][:2], runs[1][:2])
        assert runs[0][2] == list(exp.files) and runs[1][2] == list(exp.files), name
    bad = [i for i in range(N_UNSHAPED) if F.expected(T, F.unshaped_text(i), 10000, False).kind == "err"][:3]   # (the oracle's choice)
    text = F.joined([F.unshaped_text(i) for i in [0, 1] + bad])
    exp = F.expected(T, text, 10000, False)
    assert exp.kind == "err"
    path = tmp_path / "u.paf"
    path.write_bytes(text)
    runs = _cli(exe, path, [], tmp_path)
    assert runs[0] == runs[1] and runs[0][0] != 0, (runs[0][:2], runs[1][:2])
    assert exp.message in runs[0][1] and runs[0][2] == [None, None, None]
