"""K9 cannot be pinned to the reference in this image (paf_data.cpp:739+ needs ankerl/unordered_dense.h), so it gets a THIRD
reading: tests/k9_checker.py (plain Python, own shape, no oracle include) re-derives every upgraded path from the walk the heaps
gave (pinned) and the graph (pinned), checks the reference's own Debug asserts on it (:913-918), and - for every window DP of at
most 12 vertices - enumerates ALL a -> b paths and asserts that none is smaller under the QRY_SCORE_MODE order than the one taken.
CPU tier: the product's kernel bodies in the 1-lane emulation; GPU tier: the HIP path (tests below marked gpu), incl. the chain
asserts on every conversion of the C3 batch and the C5 share.  A third reading is not a pin: DESIGN.md section 2 says so.

Second half: the conversion and the selection (:1489-1649).  Every contig's main / alt / .all rows and the offset arrays are rebuilt
from the pinned intermediates and the walks and compared with the product's output; the corpus must take every branch in
K.COUNTERS, and each mutation test hands the checker a product output corrupted where one branch is taken."""
import numpy as np
import pytest

import k9_checker as K
from alignasm_amd._abi import OUT_ELEM_DTYPE

CASES = [
    # contigs, records, seed, K, dense, dup_every, shuffle, heavy_tail
    (6, 120, 42, 16, False, 7, True, False),
    (4, 250, 3, 10000, False, 0, False, False),
    (5, 90, 8, 64, False, 3, True, True),
    (2, 160, 31, 16, True, 0, False, False),
    (3, 60, 31, 10000, True, 4, True, False),
]


def _check_batch(T, hb, fetch, nc, brute_max=12):
    a = K.collect(fetch, hb.arrays["ctg_rec_off"])
    stats, bad, nconv = {}, [], 0
    for c in range(nc):
        if int(a["ctgV"][c]) == 0:
            continue
        g = K.graph_of(a, c)
        for j, (pa, pb) in enumerate(K.conversions_of(a, c)):
            nconv += 1
            bad += ["contig %d conversion %d: %s" % (c, j, x) for x in K.check_conversion(g, pa, pb, brute_max=brute_max, stats=stats)]
    return nconv, stats, bad


@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%dx%d_s%d_k%d_%s" % (c[0], c[1], c[2], c[3], "D" if c[4] else "S"))
def test_third_reading_agrees_with_the_emulated_kernel_bodies(T, case):
    nc, nr, seed, Kp, dense, dup, shuf, heavy = case
    hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup, shuffle=shuf, heavy_tail=heavy)
    T.emul_solve(hb, Kp)
    nconv, stats, bad = _check_batch(T, hb, T.emul_debug, nc)
    assert bad == [], bad[:5]
    assert nconv >= nc and stats.get("dp", 0) > 0 and stats.get("brute", 0) > 0, (nconv, stats)
    if dense:
        assert stats["brute_paths"] > stats["brute"], stats           # ... and some windows really have alternatives to rule out


def test_the_checker_notices_a_worse_path(T):
    """The checker itself: replace one window's path by a valid but longer detour (or cut the chain) and it must say so."""
    hb = T.synth(2, 160, 31, dense=True)
    T.emul_solve(hb, 16)
    a = K.collect(T.emul_debug, hb.arrays["ctg_rec_off"])
    g = K.graph_of(a, 0)
    pa, pb = K.conversions_of(a, 0)[0]
    assert K.check_conversion(g, pa, pb) == []
    assert K.check_conversion(g, pa, pb[:-1]) != []                   # does not reach dest
    assert K.check_conversion(g, pa, pb[:3] + pb[4:]) != []           # not chained
    found = False
    for t in range(1, len(pb) - 2):                                   # a shortcut u -> v for two edges u -> x -> v of the path: a valid walk that skips a record
        (u, x), (x2, v) = pb[t], pb[t + 1]
        if g.has_edge(u, v):
            worse = pb[:t] + [(u, v)] + pb[t + 2:]
            assert K.check_conversion(g, pa, worse) != []
            found = True
            break
    assert found


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES + [(40, 300, 77, 4, False, 0, False, True), (3, 700, 5, 16, True, 0, False, False)],
                         ids=lambda c: "c%dx%d_s%d_k%d_%s" % (c[0], c[1], c[2], c[3], "D" if c[4] else "S"))
def test_third_reading_agrees_with_the_hip_path(T, case):
    nc, nr, seed, Kp, dense, dup, shuf, heavy = case
    api = T.api()
    hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup, shuffle=shuf, heavy_tail=heavy)
    db = api.DeviceBatch(hb)
    res = db.solve(max_paths=Kp, keep_debug=True)
    nconv, stats, bad = _check_batch(T, hb, res.debug, nc)
    res.close(); db.close()
    assert bad == [], bad[:5]
    assert nconv >= 1 and stats.get("brute", 0) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["c3", "c5_share"])
def test_chain_asserts_hold_on_every_conversion_at_full_size(T, shape):
    """paf_data.cpp:913-918 on every converted path of the C3 batch (5 000 x 1 000, K = 4) and of the C5 per-GPU share
    (1 250 dense x 1 000, K = 16): src first, dest last, consecutive edges chained, every edge an edge of the graph."""
    api = T.api()
    if shape == "c3":
        paf, Kp = api.Paf.synth(5000, 1000, 21, no_cs=True), 4
    else:
        paf, Kp = api.Paf.synth(1250, 1000, 31, dense=True, no_cs=True), 16
    db = api.DeviceBatch(paf)
    res = db.solve(max_paths=Kp, keep_debug=True)
    rec_off = paf.batch().arrays["ctg_rec_off"]
    a = K.collect(res.debug, rec_off)
    n, nedges, bad = K.chain_invariants_batch(a["voff"], a["ctgV"], a["rowptr"], a["col"], a["cv_ctg"], a["cv_roff"], a["cv_la"], a["cv_path"], rec_off)
    st = res.stats()
    res.close(); db.close(); paf.close()
    assert bad == [], bad[:5]
    assert n == st["n_paths_converted"] and nedges > 100 * n


# ---- conversion and selection (paf_data.cpp:1489-1649): every contig's main / alt / .all rebuilt from the pinned intermediates
# and the walks, and compared with the product's output arrays.  The sequential form (one wave per contig, kb_select) keeps no
# per-conversion walks, so its outputs are checked against the walks the parallel form recovered for the same batch.
TIE_HEAVY = [(8, 40, 8, 1), (8, 40, 6, 3)]                            # contigs, records, seed, dup_every: kind-3 replacements, .all clears
FUZZ_SEEDS = range(6)


def _emul_check(T, hb, Kp, sequential=False, stats=None):
    """-> (findings, product output, checker arrays, per-contig results)."""
    rec_off = hb.arrays["ctg_rec_off"]
    out = T.emul_solve(hb, Kp)
    a = K.collect(T.emul_debug, rec_off, full=True, K=Kp)
    a["prod"] = {n: T.emul_debug(n, dt) for n, dt in (("cv_out", OUT_ELEM_DTYPE), ("cv_n", np.int32), ("cv_cov", np.int64), ("mark_time", np.int32))}
    if sequential:
        seq = T.emul_solve(hb, Kp, sequential_select=True)
        assert T.diff_outputs(out, seq, stats=False) == []
        out = seq
    bad, per = K.batch_findings(out, a, hb.arrays, lambda c: K.conversions_of(a, c, as_arrays=True), stats)
    return bad, out, a, per


@pytest.mark.parametrize("sequential", [False, True], ids=["plan", "sequential"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "c%dx%d_s%d_k%d_%s" % (c[0], c[1], c[2], c[3], "D" if c[4] else "S"))
def test_selection_reading_agrees_with_the_emulated_kernel_bodies(T, case, sequential):
    nc, nr, seed, Kp, dense, dup, shuf, heavy = case
    hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup, shuffle=shuf, heavy_tail=heavy)
    bad, out, a, per = _emul_check(T, hb, Kp, sequential)
    assert bad == [], bad[:5]
    assert sum(len(p["convs"]) for p in per.values()) >= nc


@pytest.fixture(scope="module")
def corpus(T):
    """name -> (hb, out, a, per) over the CPU corpus: the CASES, test_fuzz.make_batch batches of all three styles at K = 10 000,
    the `.all` pool-overflow batch of test_emul_vs_oracle.py and the tie-heavy batches; plus the branch counters over all of it."""
    from test_fuzz import make_batch
    batches = [("case%d" % i, T.synth(c[0], c[1], c[2], dense=c[4], dup_every=c[5], shuffle=c[6], heavy_tail=c[7]), c[3]) for i, c in enumerate(CASES)]
    batches += [("fuzz_s%d_style%d" % (s, st), make_batch(s, 40, 25, 400, st), 10000) for s in FUZZ_SEEDS for st in (0, 1, 2)]
    batches += [("pool_overflow", T.synth(3, 30, 5, dup_every=1), 10000)]
    batches += [("tie_heavy_s%d_dup%d" % (s, d), T.synth(nc, nr, s, dup_every=d, shuffle=True), 10000) for nc, nr, s, d in TIE_HEAVY]
    stats, got, bad = {}, {}, []
    for name, hb, Kp in batches:
        b, out, a, per = _emul_check(T, hb, Kp, stats=stats)
        bad += ["%s: %s" % (name, x) for x in b]
        got[name] = (hb, out, a, per)
    return got, stats, bad


def test_selection_corpus_has_no_findings_and_reaches_every_branch(corpus):
    """Zero findings over the whole corpus, and every branch of :1489-1649 the counters name taken at least once: a corpus that
    never takes a branch cannot notice a misreading of it."""
    got, stats, bad = corpus
    assert bad == [], bad[:5]
    missing = [k for k in K.COUNTERS if stats.get(k, 0) == 0]
    assert missing == [], (missing, stats)


# -- mutation tests: each corrupts the product's own output for a contig where the branch is taken; the checker must object
def _contig_with(T, corpus, counter, pred=None):
    got, _, _ = corpus
    for name, (hb, out, a, per) in got.items():
        for c in range(len(a["rec_off"]) - 1):
            st = {}
            res, _ = K.contig_outputs(a, hb.arrays, c, K.conversions_of(a, c, as_arrays=True), st)
            if st.get(counter, 0) and (pred is None or pred(hb, out, a, res, c)):
                return hb, out, a, res, c
    raise AssertionError("no contig of the corpus takes " + counter)


def _conv_rows(a, c, t):
    """The product's rows of conversion t of contig c (cv_out), flags resolved as the product does (mark_time)."""
    j = int(a["conv_off"][c]) + t
    p = a["prod"]
    r0 = int(a["cv_roff"][j])
    rows = p["cv_out"][r0:r0 + int(p["cv_n"][j])].copy()
    rows["is_alt"] = p["mark_time"][int(a["rec_off"][c]) + rows["is_alt"]] > t
    return rows


def _with_rows(out, key, c, rows):
    """out with contig c's `key` (main / alt) rows replaced."""
    o = dict(out)
    off = out[key + "_off"]
    o[key] = np.concatenate([out[key][:off[c]], rows.astype(out[key].dtype), out[key][off[c + 1]:]])
    o[key + "_off"] = off.copy()
    o[key + "_off"][c + 1:] += len(rows) - (off[c + 1] - off[c])
    return o


def _with_all(out, c, paths):
    """out with contig c's `.all` list replaced by `paths` (a list of row arrays)."""
    o = dict(out)
    po, eo = out["all_path_off"], out["all_elem_off"]
    p0, p1 = int(po[c]), int(po[c + 1])
    lens = list(np.diff(eo[:p0])) + [len(x) for x in paths] + list(np.diff(eo[p1:]))
    o["all_elem_off"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    o["all_path_off"] = po.copy()
    o["all_path_off"][c + 1:] += len(paths) - (p1 - p0)
    o["all"] = np.concatenate([out["all"][:eo[p0]]] + [x.astype(out["all"].dtype) for x in paths] + [out["all"][eo[p1]:]])
    return o


def _findings(hb, out, a):
    return K.batch_findings(out, a, hb.arrays, lambda c: K.conversions_of(a, c, as_arrays=True))[0]


def test_checker_rejects_a_clip_from_the_wrong_pair(T, corpus):
    hb, out, a, res, c = _contig_with(T, corpus, "clip_end", lambda hb, out, a, res, c: res["convs"][res["pick"][0]]["clip_e"].any())
    assert _findings(hb, out, a) == []
    i = int(np.nonzero(res["convs"][res["pick"][0]]["clip_e"])[0][0])
    m = out["main"][out["main_off"][c]:out["main_off"][c + 1]].copy()
    vb, V = int(a["voff"][c]), int(a["ctgV"][c])
    pairs = a["v_slot"][vb:vb + V - 2][a["v_i"][vb:vb + V - 2] != a["v_j"][vb:vb + V - 2]]
    other = next(int(a["ov_peq"][s]) for s in pairs if int(a["ov_peq"][s]) != int(m["qe"][i]))   # another pair's end cut
    m["qe"][i] = other
    assert _findings(hb, _with_rows(out, "main", c, m), a) != []


def test_checker_rejects_flags_from_the_upgraded_path(T, corpus):
    hb, out, a, res, c = _contig_with(T, corpus, "alt_never_marked", lambda hb, out, a, res, c: res["main"]["is_alt"].any())
    m = out["main"][out["main_off"][c]:out["main_off"][c + 1]].copy()
    assert m["is_alt"].any()
    m["is_alt"] = 0                                                   # every record of the upgraded path counted as seen
    assert _findings(hb, _with_rows(out, "main", c, m), a) != []


def test_checker_rejects_marks_not_carried_over(T, corpus):
    def where(hb, out, a, res, c):
        main, alt, allp = res["pick"]
        return alt >= 0 and ((res["alt"]["is_alt"] == 0) & ~res["convs"][alt]["own"][res["alt"]["ctg_index"]]).any()
    hb, out, a, res, c = _contig_with(T, corpus, "kept_by_earlier_mark", where)
    alt = res["pick"][1]
    r = out["alt"][out["alt_off"][c]:out["alt_off"][c + 1]].copy()
    r["is_alt"] = ~res["convs"][alt]["own"][r["ctg_index"]]           # marks of the alt walk alone
    assert _findings(hb, _with_rows(out, "alt", c, r), a) != []


def test_checker_rejects_the_first_tie_as_main(T, corpus):
    hb, out, a, res, c = _contig_with(T, corpus, "main_from_tie")
    assert res["pick"][0] > 0
    assert _findings(hb, _with_rows(out, "main", c, _conv_rows(a, c, 0)), a) != []


def test_checker_rejects_an_all_list_not_cleared(T, corpus):
    hb, out, a, res, c = _contig_with(T, corpus, "all_cleared")
    cov = a["prod"]["cv_cov"][int(a["conv_off"][c]):int(a["conv_off"][c + 1])]
    best, keep = int(cov[0]), []
    for t, (k, kind) in enumerate(res["plan"]):                       # :1603-1609 without the clear()
        if kind == 1 and cov[t] > best:
            best = int(cov[t])
        elif kind == 1 and cov[t] == best:
            keep.append(t)
    assert len(keep) > len(res["all"])
    assert _findings(hb, _with_all(out, c, [_conv_rows(a, c, t) for t in keep]), a) != []


def test_checker_rejects_path_0_in_the_all_list(T, corpus):
    hb, out, a, res, c = _contig_with(T, corpus, "all_nonempty")
    po, eo = out["all_path_off"], out["all_elem_off"]
    mine = [out["all"][eo[p]:eo[p + 1]] for p in range(int(po[c]), int(po[c + 1]))]
    assert _findings(hb, _with_all(out, c, [_conv_rows(a, c, 0)] + mine), a) != []


def test_checker_rejects_the_last_kind_2_as_alt(T, corpus):
    hb, out, a, res, c = _contig_with(T, corpus, "k3_replaced")
    last2 = max(t for t, (k, kind) in enumerate(res["plan"]) if kind == 2)
    assert res["pick"][1] != last2
    assert _findings(hb, _with_rows(out, "alt", c, _conv_rows(a, c, last2)), a) != []


def test_checker_rejects_kind_3_taken_on_equal_coverage(T, corpus):
    def where(hb, out, a, res, c):
        return any(kind == 3 and cv["cov"] == res["convs"][res["pick"][1]]["cov"] and K._rows_diff(cv["rows"], res["alt"]) is not None
                   for (k, kind), cv in zip(res["plan"], res["convs"]))
    hb, out, a, res, c = _contig_with(T, corpus, "k3_equal_cov", where)
    alt = res["pick"][1]
    t = next(t for t, ((k, kind), cv) in enumerate(zip(res["plan"], res["convs"]))
             if t > alt and kind == 3 and cv["cov"] == res["convs"][alt]["cov"] and K._rows_diff(cv["rows"], res["alt"]) is not None)
    assert _findings(hb, _with_rows(out, "alt", c, _conv_rows(a, c, t)), a) != []


def _hip_check(T, src, inp, Kp, sequential=False, stats=None):
    """A keep_debug solve supplies the walks and the intermediates; the outputs checked are those of a plain solve (plan form
    or sequential form), which must also equal the debug solve's - the debug path compacts its arena differently and must not
    be what makes the check pass.  Returns (findings, #conversions)."""
    api = T.api()
    db = api.DeviceBatch(src)
    res = db.solve(max_paths=Kp, keep_debug=True)
    dbg_out = res.fetch()
    a = K.collect(res.debug, inp["ctg_rec_off"], full=True, K=Kp)
    res.close(); db.close()
    out = api.solve_batch(src, max_paths=Kp, sequential_select=sequential)
    assert T.diff_outputs(out, dbg_out, stats=False) == []
    bad, per = K.batch_findings(out, a, inp, lambda c: K.conversions_of(a, c, as_arrays=True), stats)
    return bad, sum(len(p["convs"]) for p in per.values())


@pytest.mark.gpu
@pytest.mark.parametrize("sequential", [False, True], ids=["plan", "sequential"])
@pytest.mark.parametrize("case", CASES + [(40, 300, 77, 4, False, 0, False, True), (3, 700, 5, 16, True, 0, False, False)],
                         ids=lambda c: "c%dx%d_s%d_k%d_%s" % (c[0], c[1], c[2], c[3], "D" if c[4] else "S"))
def test_selection_reading_agrees_with_the_hip_path(T, case, sequential):
    nc, nr, seed, Kp, dense, dup, shuf, heavy = case
    hb = T.synth(nc, nr, seed, dense=dense, dup_every=dup, shuffle=shuf, heavy_tail=heavy)
    bad, nconv = _hip_check(T, hb, hb.arrays, Kp, sequential)
    assert bad == [], bad[:5]
    assert nconv >= nc


FULL = {                                                              # contigs, records, seed, K, generator options (bench.py's)
    "c3": (5000, 1000, 21, 4, {}),
    "c3_dup3": (5000, 1000, 21, 4, {"dup_every": 3}),
    "c3_heavy_tail": (5000, 1000, 21, 4, {"heavy_tail": True}),
    "c5_share": (1250, 1000, 31, 16, {"dense": True}),
    "shipped_k": (200, 1000, 41, 10000, {}),
}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(FULL))
def test_selection_reading_on_every_contig_at_full_size(T, shape):
    """plan, walk_ok, convert and select on every contig of the full batches, every output row and offset compared."""
    import time
    nc, nr, seed, Kp, kw = FULL[shape]
    api = T.api()
    paf = api.Paf.synth(nc, nr, seed, no_cs=True, **kw)
    t0 = time.time()
    stats = {}
    bad, nconv = _hip_check(T, paf, paf.batch().arrays, Kp, stats=stats)
    paf.close()
    print("%s: %d conversions checked in %.1f s; branch counts %r" % (shape, nconv, time.time() - t0, stats))
    assert bad == [], bad[:5]
    assert nconv >= nc // 2
