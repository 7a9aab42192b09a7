"""Coordinates up to the 2^40 limit, CPU tier: the wide corpus of tests/wide_cases.py through the kernel bodies (1-lane host
emulation), the oracle, the real reference prefix (recorded, and live where it is built), the K9 checker and the host I/O.

The rest of the suite stays below 2^31, so every int64 there has a zero high word.  Here coordinates straddle 2^31 and 2^32,
sit at 5 * 2^32 + 7 and at 2^40 - 1, edge query weights and k-walk score sums exceed 2^32, capped reference gaps have raw
values above 2^32, and distinct score sums of one contig share their low 32 bits.  The GPU tier runs the same corpus on the
card: tests/test_gpu_wide_coords.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import k9_checker as K
import wide_cases as W
from alignasm_amd._abi import OUT_ELEM_DTYPE, BatchOut, HostBatch, Opts


@pytest.fixture(scope="module")
def corpus(T):
    return W.corpus(T)


def test_corpus_reaches_the_wide_cases(T, corpus):
    """The corpus really holds what it is for: every count of wide_cases.coverage above zero, every batch inside [0, 2^40),
    and each of the five checked fields at exactly 2^40 - 1 somewhere."""
    n = W.coverage(T, corpus)
    assert all(v > 0 for v in n.values()), n
    at_top = set()
    for name, hb in corpus:
        for k in W.CHECKED:
            a = hb.arrays[k]
            assert a.min() >= 0 and a.max() < W.LIMIT, (name, k)
            if a.max() == W.TOP:
                at_top.add(k)
    assert at_top == set(W.CHECKED), at_top
    names, hb = W.crafted(top=True)
    off = hb.arrays["ctg_rec_off"]
    for k in W.CHECKED:                                        # ... each in a contig of its own name
        c = names.index("top_" + k)
        assert hb.arrays[k][off[c]:off[c + 1]].max() == W.TOP, k


def test_shift_helpers(T):
    """The metamorphic pair itself: shift moves exactly the query and the reference fields, shift_out exactly the elements."""
    hb = T.synth(2, 20, 3)
    s = W.shift(hb, 5, -7)
    for k, a in hb.arrays.items():
        d = 5 if k in W.Q_FIELDS else -7 if k in W.R_FIELDS else 0
        assert np.array_equal(s.arrays[k], a + d), k
    out = T.oracle_solve(hb, 4)
    so = W.shift_out(out, 5, -7)
    for key in ("main", "alt", "all"):
        for f, d in (("qs", 5), ("qe", 5), ("rs", -7), ("re", -7), ("ctg_index", 0), ("is_alt", 0)):
            assert np.array_equal(so[key][f], out[key][f] + d), (key, f)
    assert T.diff_outputs(out, so) == [k for k in ("main", "alt", "all") if len(out[k])] and len(out["main"]) > 0


@pytest.mark.parametrize("K_,nsl", [(10000, False), (10000, True), (3, False), (3, True)])
def test_emulation_matches_oracle_on_wide_corpus(T, corpus, K_, nsl):
    for name, hb in corpus:
        want = T.oracle_solve(hb, K_, nsl)
        assert (want["status"] == 0).all(), name
        assert T.diff_outputs(want, T.emul_solve(hb, K_, nsl)) == [], (name, K_, nsl)


HOOKS = [dict(chain="all"), dict(chain="none"), dict(chain="half"), dict(heap_waves="all"), dict(heap_waves="none"),
         dict(sequential_select=True), dict(graph_launches=True), dict(enum_heap=True)]


@pytest.mark.parametrize("hooks", HOOKS, ids=lambda h: "-".join(f"{k}={v}" for k, v in h.items()))
def test_emulation_launch_forms_match_oracle_on_wide_corpus(T, corpus, hooks):
    for name, hb in corpus:
        for K_, nsl in ((10000, False), (3, True)):
            assert T.diff_outputs(T.oracle_solve(hb, K_, nsl), T.emul_solve(hb, K_, nsl, **hooks)) == [], (name, K_, nsl)


def _shift_cases(T):
    out = W.shifted(T)
    out += [(n + "+5g", hb, 5 * (1 << 32) + 7, 5 * (1 << 32) + 7) for n, hb in W.wide_fuzz(seeds=(0,))]
    return out


@pytest.mark.parametrize("which", ["oracle", "emulation"])
def test_solve_commutes_with_shift(T, which):
    """solve(shift(b, dq, dr)) == shift_out(solve(b), dq, dr), for every offset of the corpus and for the wide fuzz moved further."""
    solve = T.oracle_solve if which == "oracle" else T.emul_solve
    n = 0
    for name, hb, dq, dr in _shift_cases(T):
        for K_, nsl in ((10000, False), (3, True)):
            base = solve(hb, K_, nsl)
            assert T.diff_outputs(W.shift_out(base, dq, dr), solve(W.shift(hb, dq, dr), K_, nsl)) == [], (name, K_, nsl)
            n += len(base["main"])
    assert n > 1000


def test_k9_checker_accepts_every_wide_contig(T, corpus):
    """tests/k9_checker.py's independent reading of K9 (conversions, selection, main / alt / .all) on every contig."""
    stats, nconv = {}, 0
    for name, hb in corpus:
        out = T.emul_solve(hb, 10000)
        a = K.collect(T.emul_debug, hb.arrays["ctg_rec_off"], full=True, K=10000)
        a["prod"] = {n: T.emul_debug(n, dt) for n, dt in (("cv_out", OUT_ELEM_DTYPE), ("cv_n", np.int32), ("cv_cov", np.int64), ("mark_time", np.int32))}
        bad, per = K.batch_findings(out, a, hb.arrays, lambda c: K.conversions_of(a, c, as_arrays=True), stats)
        assert bad == [], (name, bad[:4])
        nconv += sum(len(p["convs"]) for p in per.values())
    assert nconv > 500


# ---- the real reference prefix ------------------------------------------------------------------------------------
@pytest.mark.ref
def test_oracle_matches_reference_prefix_on_wide_batches(T, corpus):
    if T.ref_prefix(True) is None:
        pytest.skip("oracle/_ref/libaasm_ref_prefix*.so not built (no /root/reference on this box and no prebuilt .so)")
    from test_ref_prefix import _diff_oracle
    nd = 0
    for name, hb in corpus:
        for nsl in (False, True):
            bad, a, _ = _diff_oracle(T, hb, range(hb.n_contigs), nsl)
            assert bad == [], (name, nsl, bad[:4])
            nd += a
    assert nd > 100000


@pytest.fixture(scope="module")
def V(T):
    return T.RefPrefixVectors(os.path.join(T.GOLDEN, "ref_prefix_wide.npz"))


def test_wide_fixture_is_wide(T, V):
    assert len(V.tags) >= 12
    n_dist = n_sum32 = n_wq32 = big = 0
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        big += int(hb.arrays["qry_total"].max() >= 1 << 32)
        for c in range(hb.n_contigs):
            r = V.contig(tag, c)
            if r:
                n_dist += len(r["kd_qry"])
                n_sum32 += int((r["kd_qry"] + r["kd_ref"] >= 1 << 32).sum())
                n_wq32 += int((r["csr_w_qry"] >= 1 << 32).sum())
    assert big >= 8 and n_dist > 2000 and n_sum32 > 1000 and n_wq32 > 100, (big, n_dist, n_sum32, n_wq32)


def test_oracle_matches_recorded_wide_reference_prefix(T, V):
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        for c in range(hb.n_contigs):
            r = V.contig(tag, c)
            if not r:
                continue
            o = T.oracle_debug(hb, c, 10000, nsl)
            assert len(o["kd_qry"]) == r["kfound"][0], (tag, c)
            for n in T.PREFIX_NAMES:
                want = r[n]
                assert np.array_equal(o[n][:len(want)] if n.startswith("kd_") else o[n], want), (tag, c, n)


def test_kernel_bodies_match_recorded_wide_reference_prefix(T, V):
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        for K_ in ((10000, 4) if full else (64,)):
            T.emul_solve(hb, K_, nsl)
            assert T.diff_intermediates(hb, T.emul_debug, K_, nsl, expect=lambda c: V.contig(tag, c)) == [], (tag, K_)


# ---- host I/O ------------------------------------------------------------------------------------------------------
def shift_paf(text, dq, dr, dlen=0):
    """PAF text with query columns (length, start, end) moved by dq and reference columns (start, end) by dr; the reference
    length column grows by dlen.  cs tags are relative and stay."""
    rows = []
    for ln in text.decode().split("\n"):
        if not ln:
            rows.append(ln)
            continue
        f = ln.split("\t")
        f[1], f[2], f[3] = (str(int(x) + dq) for x in f[1:4])
        f[6] = str(int(f[6]) + dlen)
        f[7], f[8] = (str(int(x) + dr) for x in f[7:9])
        rows.append("\t".join(f))
    return "\n".join(rows).encode()


def _paf_offsets():
    d11, d13 = 10 ** 10, 10 ** 12                           # 11- and 13-digit coordinates (inside the solver's 2^40 ~ 1.1e12)
    d18, d19 = 10 ** 17, 10 ** 18                           # across the 18 / 19-digit boundary of fast_i64 (reader only)
    return {"x32": ((1 << 32) - 20000, (1 << 32) - 3 * 10 ** 7), "d11": (d11, d11 + 7), "d13": (d13 + 5, d13 - 123456789),
            "d18": (d18 - 20000, d18 - 2 * 10 ** 7), "d19": (d19 - 20000, d19 - 2 * 10 ** 7)}


@pytest.mark.parametrize("name", list(_paf_offsets()))
def test_reader_matches_io_oracle_on_wide_text(T, name):
    """11- to 13-digit coordinates, and 18- and 19-digit numbers at the fast_i64 / strtoll boundary of the reader."""
    api, io = T.api(), T.io_oracle()
    dq, dr = _paf_offsets()[name]
    text = shift_paf(api.Paf.synth(5, 60, 3, dup_every=4, shuffle=True).to_text(), dq, dr, dlen=dr)
    digits = {len(x) for ln in text.decode().splitlines() for x in ln.split("\t")[1:9] if x.isdigit()}
    if name == "d18":
        assert {17, 18} <= digits
    if name == "d19":
        assert {18, 19} <= digits
    want = io.to_arrays(io.read_paf(text))
    paf = api.Paf.parse(text)
    got = paf.batch().arrays
    for k, a in want.items():
        assert np.array_equal(np.asarray(a, np.int64), np.asarray(got[k], np.int64)), (name, k)
    paf.close()


@pytest.mark.parametrize("name", ["x32", "d11", "d13"])
def test_writers_match_io_oracle_on_wide_results(T, tmp_path, name):
    """process_output / process_max_output with coordinates of 10 to 13 digits (clipped rows included)."""
    api, io = T.api(), T.io_oracle()
    dq, dr = _paf_offsets()[name]
    text = shift_paf(api.Paf.synth(12, 120, 21, dup_every=6).to_text(), dq, dr, dlen=dr)
    st = io.read_paf(text)
    hb = T.io_oracle_batch(st)
    assert hb.arrays["qry_total"].max() > 1 << 32 or name == "x32"
    assert all(hb.arrays[k].max() < 1 << 40 for k in ("qry_total", "ref_str", "ref_end"))
    want = io.render_outputs(st, T.oracle_solve(hb, 64))
    paf = api.Paf.parse(text)
    out = BatchOut()
    assert T.oracle().oracle_solve_batch(C.byref(hb.view), C.byref(Opts(64, 0, 0, 0, 0)), 2, C.byref(out)) == 0
    paths = [str(tmp_path / n) for n in ("x.aln.paf", "x.aln.alt.paf", "x.aln.all.paf")]
    paf.write_outputs(out, *paths)
    T.oracle().oracle_free_out(C.byref(out))
    got = [open(p, "rb").read() for p in paths]
    assert got == list(want)
    assert want[0].count(b"\n") > 100


@pytest.mark.parametrize("value", [1 << 40, -1], ids=["2^40", "-1"])
def test_cli_refuses_a_coordinate_outside_the_range(T, tmp_path, value):
    """The binary's host-side guard runs before any device work: a non-zero exit and a message naming the record."""
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    text = shift_paf(T.api().Paf.synth(3, 6, 3).to_text(), 1 << 33, 1 << 33)
    lines = text.decode().split("\n")
    f = lines[8].split("\t")
    if value < 0:
        f[2] = str(value)                                      # qry_str
    else:
        f[1] = str(value)                                      # qry_total
    lines[8] = "\t".join(f)
    p = tmp_path / "w.paf"
    p.write_text("\n".join(lines))
    r = subprocess.run([exe, str(p)], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "record 8" in r.stderr and "2^40" in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / "w.aln.paf").exists()
