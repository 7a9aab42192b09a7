"""Coordinates up to the 2^40 limit, GPU tier: the HIP path on the wide corpus of tests/wide_cases.py.

The GPU build splits 64-bit values into 32-bit pieces in many places (wave shuffles and broadcasts, readlane pairs, K7's heap
node keys held as quads, the packed in-edge record, K9's candidate quads, K8's default queue with its DPP / swizzle / bpermute
moves and its far-tier threshold).  The 1-lane emulation of the CPU tier runs none of the multi-lane paths, so only the card
can show that those joins keep the high word.  Every solve here must equal the oracle, and a shifted batch must also equal
wide_cases.shift_out of the HIP solve of the unshifted one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import wide_cases as W
from alignasm_amd._abi import HostBatch
from test_fuzz import make_batch
from test_wide_coords import shift_paf

pytestmark = pytest.mark.gpu

G32 = 1 << 32
FORMS = [{}, dict(chain="all"), dict(chain="none"), dict(chain="half"), dict(heap_waves="all"), dict(heap_waves="none"),
         dict(sequential_select=True), dict(graph_launches=True), dict(enum_heap=True), dict(grid_order=True), dict(enum_small=True),
         dict(heap_waves="all", heap_block_waves=4), dict(heap_waves="all", heap_block_waves=8), dict(heap_waves="all", heap_block_waves=16)]
SETTINGS = ((10000, False), (3, True))


@pytest.fixture(scope="module")
def corpus(T):
    """name -> (HostBatch, {(K, nsl): oracle result}, (base name, dq, dr) or None)."""
    out = {}
    for n, hb in W.corpus(T):
        out[n] = [hb, {s: T.oracle_solve(hb, *s) for s in SETTINGS}, None]
    for n, base, dq, dr in W.shifted(T):
        out[n][2] = (base, dq, dr)
    return out


def test_hip_matches_oracle_and_shift_on_wide_corpus_in_every_launch_form(T, corpus):
    api = T.api()
    n_checked = 0
    for name, (hb, want, sh) in corpus.items():
        db = api.DeviceBatch(hb)
        base = {}
        if sh is not None:
            bdb = api.DeviceBatch(sh[0])
            for K, nsl in SETTINGS:
                r = bdb.solve(max_paths=K, non_skip_linkable=nsl)
                base[(K, nsl)] = W.shift_out(r.fetch(), sh[1], sh[2])
                r.close()
            bdb.close()
        for hooks in FORMS:
            for K, nsl in SETTINGS:
                r = db.solve(max_paths=K, non_skip_linkable=nsl, **hooks)
                got = r.fetch()
                r.close()
                assert T.diff_outputs(want[(K, nsl)], got) == [], (name, hooks, K, nsl)
                if base:
                    assert T.diff_outputs(base[(K, nsl)], got) == [], (name, hooks, K, nsl, "shift")
                n_checked += 1
        db.close()
    assert n_checked == len(corpus) * len(FORMS) * len(SETTINGS)


def test_hip_intermediates_on_wide_batches(T, corpus):
    """K1 ... K8 array by array (weights, d / best, heap node keys, all 10 000 distances) against the oracle."""
    api = T.api()
    names = ["crafted", "crafted_top", "wf33_s0_y0", "wf39_s0_y2", "syn+x32", "dense+5g", "fz1+top"]
    for name in names:
        hb = corpus[name][0]
        db = api.DeviceBatch(hb)
        for hooks in ({}, dict(chain="none", heap_waves="all"), dict(chain="none", heap_waves="none")):
            res = db.solve(max_paths=10000, keep_debug=True, **hooks)
            bad = T.diff_intermediates(hb, res.debug, 10000)
            res.close()
            assert bad == [], (name, hooks, bad[:6])
        db.close()


@pytest.mark.parametrize("heap_waves,chain", [("auto", "auto"), ("all", "auto"), ("none", "auto"), ("auto", "none"), ("auto", "half")])
def test_hip_intermediates_match_recorded_wide_reference_prefix(T, heap_waves, chain):
    """tests/golden/ref_prefix_wide.npz: what the reference's own statements computed on wide batches."""
    api = T.api()
    V = T.RefPrefixVectors(os.path.join(T.GOLDEN, "ref_prefix_wide.npz"))
    for tag in V.tags:
        hb, nsl, full = V.batch(tag)
        db = api.DeviceBatch(hb)
        for K in ((10000, 4) if full else (64, 1)):
            res = db.solve(max_paths=K, non_skip_linkable=nsl, keep_debug=True, heap_waves=heap_waves, chain=chain)
            bad = T.diff_intermediates(hb, res.debug, K, nsl, expect=lambda c: V.contig(tag, c))
            res.close()
            assert bad == [], (tag, K, bad[:6])
        db.close()


def test_k8_queue_forms_agree_on_wide_sums(T):
    """K8 at K = 10 000 with score sums above 2^32: the default queue (sorted front, runs, far tier split by a threshold on the
    sum) and the d-ary heap pop the same distances, equal to the oracle's."""
    api = T.api()
    batches = [W.shift(T.synth(3, 300, 5, dup_every=3), G32 - 10 ** 6, 3 * G32), make_batch(77, 4, 60, W.WIDE_L[1], 0),
               make_batch(78, 4, 60, W.WIDE_L[0], 2), W.shift(T.synth(2, 200, 31, dense=True), 7 * G32 + 5, G32 + (1 << 31))]
    n_far = 0
    for hb in batches:
        db = api.DeviceBatch(hb)
        got = {}
        for form in ("runs", "heap"):
            res = db.solve(max_paths=10000, keep_debug=True, enum_heap=(form == "heap"))
            assert T.diff_intermediates(hb, res.debug, 10000) == [], form
            nc = hb.n_contigs
            got[form] = (res.debug("kfound", np.int32)[:nc].copy(), res.debug("kd", T.DIST_DT)[:nc * 10000].copy(), res.fetch())
            res.close()
        db.close()
        a, b = got["runs"], got["heap"]
        assert np.array_equal(a[0], b[0])
        for c in range(hb.n_contigs):
            n = int(a[0][c])
            s = a[1]["qry"][c * 10000:c * 10000 + n] + a[1]["ref"][c * 10000:c * 10000 + n]
            n_far += int((s >= G32).sum() > 0 and n > 1000)
            for f in ("qry", "ref", "anom", "qnz", "qtot"):
                assert np.array_equal(a[1][f][c * 10000:c * 10000 + n], b[1][f][c * 10000:c * 10000 + n]), (c, f)
        assert T.diff_outputs(a[2], b[2]) == []
        assert T.diff_outputs(T.oracle_solve(hb, 10000), a[2]) == []
    assert n_far >= 4                                           # long pop sequences (the far tier in use) with sums above 2^32


def test_two_contigs_per_wave_on_wide_fuzz(T):
    """2 700 wide fuzz contigs (above 2 560: the sweeps run two contigs per wave, 32 lanes each)."""
    api = T.api()
    for seed, L, style in ((7, W.WIDE_L[0], 0), (8, W.WIDE_L[1], 2)):
        hb = make_batch(seed, 2700, 14, L, style)
        for K, nsl in SETTINGS:
            assert T.diff_outputs(T.oracle_solve(hb, K, nsl, threads=16), api.solve_batch(hb, max_paths=K, non_skip_linkable=nsl)) == [], (seed, K)


def test_giant_contig_across_2_32(T):
    """One contig of 20 000 records moved across 2^32 (the chain class: aasm_k67_chain), and in the three launches."""
    api = T.api()
    base = T.synth(1, 20000, 7)
    dq, dr = W.offsets(base)["x32"]
    hb = W.shift(base, dq, dr)
    want = T.oracle_solve(hb, 4)
    shifted_base = W.shift_out(api.solve_batch(base, max_paths=4), dq, dr)
    for hooks in ({}, dict(chain="none")):
        got = api.solve_batch(hb, max_paths=4, **hooks)
        assert T.diff_outputs(want, got) == [] and T.diff_outputs(shifted_base, got) == [], hooks


@pytest.mark.parametrize("shape", ["c3", "c5_share"])
def test_full_size_batch_across_2_32(T, shape):
    """C3 (5 000 x 1 000, K = 4) and the C5 share (1 250 dense x 1 000, K = 16: kb_heap_mw) moved across 2^32, whole batch."""
    api = T.api()
    args, K = ((5000, 1000, 21, False), 4) if shape == "c3" else ((1250, 1000, 31, True), 16)
    paf = api.Paf.synth(*args[:3], dense=args[3], no_cs=True)
    base = paf.batch()
    paf.close()
    dq, dr = W.offsets(base)["x32"]
    hb = W.shift(base, dq, dr)
    got = api.solve_batch(hb, max_paths=K)
    assert T.diff_outputs(W.shift_out(api.solve_batch(base, max_paths=K), dq, dr), got) == []
    assert T.diff_outputs(T.oracle_solve(hb, K, threads=16), got, stats=False) == []


def test_device_cs_path_on_shifted_text(T):
    """K0 on cs tags of records moved across 2^32 (the tags are relative): the cs-text solve equals the host-range solve and
    the oracle."""
    api = T.api()
    base = api.Paf.synth(30, 150, 9, dup_every=4, shuffle=True).to_text()
    text = shift_paf(base, G32 - 20000, G32 - 3 * 10 ** 7, dlen=G32)
    host_paf, dev_paf = api.Paf.parse(text), api.Paf.parse(text, device_ranges=True)
    hb = host_paf.batch()
    assert hb.arrays["qry_str"].min() < G32 < hb.arrays["qry_end"].max()
    for K in (16, 10000):
        want = T.oracle_solve(hb, K)
        a = api.solve_batch(host_paf, max_paths=K)
        b = api.solve_batch(dev_paf, max_paths=K)
        assert T.diff_outputs(want, a) == [] and T.diff_outputs(want, b) == [], K


def test_resident_batch_flags_2_40_and_solves_2_40_minus_1(T):
    api = T.api()
    hb = W.shift(T.synth(5, 40, 3), 3 * G32, 3 * G32)
    for value, status in ((W.LIMIT, -5), (W.TOP, 0)):
        for field in W.CHECKED:
            a = {k: v.copy() for k, v in hb.arrays.items()}
            r = int(a["ctg_rec_off"][2]) + 3
            a[field][r] = value
            if field == "qry_str":
                a["qry_end"][r] = value                          # keep qs <= qe
            if field in ("qry_end", "qry_str"):
                a["qry_total"][r] = value
            bad = HostBatch(a)
            db = api.DeviceBatch(bad)
            res = db.solve(max_paths=8)
            out = res.fetch()
            res.close(); db.close()
            assert list(out["status"]) == [0, 0, status, 0, 0], (field, value)
            if status == 0:
                assert T.diff_outputs(T.oracle_solve(bad, 8), out) == [], field
                continue
            want = T.oracle_solve(hb, 8)
            assert out["main_off"][3] == out["main_off"][2]
            for c in (0, 1, 3, 4):
                for k in ("main", "alt"):
                    o, wo = out[k + "_off"], want[k + "_off"]
                    assert np.array_equal(want[k][wo[c]:wo[c + 1]], out[k][o[c]:o[c + 1]]), (field, c, k)


def test_export_equals_fetch_on_wide_batches(T, corpus):
    """to_torch() (the 8-byte aasm_pack_* copies) equals fetch() with edited coordinates above 2^32."""
    import torch
    api = T.api()
    n_wide = 0
    for name in ("crafted", "crafted_top", "wf39_s0_y0", "syn+5g", "dense+x32"):
        hb = corpus[name][0]
        db = api.DeviceBatch(hb)
        for K in (10000, 3):
            res = db.solve(max_paths=K)
            d = res.to_torch()
            torch.cuda.current_stream(res.device).synchronize()
            got = api.torch_to_numpy(d)
            want = res.fetch()
            res.close()
            for k in ("main_off", "alt_off", "all_path_off", "all_elem_off", "main", "alt", "all", "status"):
                assert want[k].tobytes() == got[k].tobytes(), (name, K, k)
            n_wide += int((want["all"]["qe"] >= G32).sum())
        db.close()
    assert n_wide > 100


def test_dijkstra_on_wide_weights(T):
    """aasm_sssp_dijkstra against the oracle's dijkstra() on digraphs with cycles and weights in [0, 2^39), including graphs
    whose path sums tie in the low 32 bits only."""
    from test_dijkstra import random_digraph, run
    api = T.api()
    rng = np.random.default_rng(2040)
    gs = []
    for n, p in ((8, 0.3), (25, 0.15), (60, 0.08), (120, 0.04)):
        for kind in range(3):
            rp, col, w = random_digraph(rng, n, p)
            w = w.reshape(-1, 5)
            if kind == 0:                                        # any weight below 2^39
                w[:, 0] = rng.integers(0, 1 << 39, len(w)); w[:, 1] = rng.integers(0, 1 << 39, len(w))
            else:                                                # small weights plus multiples of 2^32: sums equal modulo 2^32
                w[:, 0] += rng.integers(0, 4, len(w)) * G32; w[:, 1] += rng.integers(0, 3, len(w)) * (G32 if kind == 1 else 1 << 31)
            gs.append((n, rp, col, w.reshape(-1).copy(), int(rng.integers(0, n))))
    voff = np.concatenate([[0], np.cumsum([g[0] for g in gs])]).astype(np.int64)
    rowptr = np.concatenate([[0]] + [g[1][1:] + sum(len(h[2]) for h in gs[:i]) for i, g in enumerate(gs)]).astype(np.int64)
    col = np.concatenate([g[2] for g in gs]).astype(np.int32)
    w = np.concatenate([g[3] for g in gs])
    d, prev = api.sssp_dijkstra(voff, rowptr, col, w, [g[4] for g in gs])
    ties = 0
    for i, (n, rp, cl, ww, src) in enumerate(gs):
        wd, wp = run(T.oracle(), "oracle_", n, rp, cl, ww, src)
        assert np.array_equal(d[voff[i]:voff[i + 1]].reshape(n, 5), wd), i
        assert np.array_equal(prev[voff[i]:voff[i + 1]], wp), i
        s = wd[:, 0] + wd[:, 1]
        s = np.unique(s[wd[:, 0] >= 0])
        ties += len(s) - len(np.unique(s & 0xFFFFFFFF))
    assert ties > 0


# ---- K8's order key (aasm_debug_predicates bit 5: qe_less on entries built with qe_key2) ------------------------------
def _predicates(api, a, b):
    """aasm_debug_predicates on n pairs of 5-tuples (two (n, 5) arrays) -> n result bytes."""
    a, b = np.ascontiguousarray(a, np.int64), np.ascontiguousarray(b, np.int64)
    assert a.shape == b.shape and a.shape[1:] == (5,)
    got = np.zeros(len(a), np.uint8)
    rc = api.LIB.aasm_debug_predicates(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), C.c_int64(len(a)), got.ctypes.data_as(C.c_void_p), 0)
    assert rc == 0, api.LIB.aasm_last_error()
    return got


def _exact_less(x, y):
    """K8's order on distances of real walks in exact integers: score sum, anom, then the ratio qnz / qtot, higher first."""
    sx, sy = x[0] + x[1], y[0] + y[1]
    if sx != sy:
        return sx < sy
    if x[2] != y[2]:
        return x[2] < y[2]
    return x[3] * max(y[4], 1) > y[3] * max(x[4], 1)


def _farey_pairs(rng, n):
    """Neighbours a/b < c/d in the Farey sequence of order 2^20 - 1 (b c - a d = 1): the closest ratios qtot < 2^20 allows."""
    out, M = [], (1 << 20) - 1
    while len(out) < n:
        b = int(rng.integers(2, M + 1)) if len(out) % 2 else int(rng.integers(M - 4096, M + 1))
        a = int(rng.integers(1, b))
        if np.gcd(a, b) != 1:
            continue
        d = (-pow(a, -1, b)) % b
        d += b * int(rng.integers(0, max(1, (M - d) // b + 1)))
        if d == 0 or d > M:
            continue
        c = (1 + a * d) // b
        assert b * c - a * d == 1 and c <= d
        out.append((a, b, c, d))
    return out


def test_k8_order_key_on_farey_neighbours_and_low_word_ties(T):
    api = T.api()
    rng = np.random.default_rng(20)
    A, B = [], []
    for a, b, c, d in _farey_pairs(rng, 3000):
        s = int(rng.integers(0, 1 << 41))
        q = int(rng.integers(0, s + 1))
        anom = int(rng.integers(0, 3))
        x, y = [q, s - q, anom, a, b], [s - q, q, anom, c, d]
        A += [x, y, x]; B += [y, x, [q, s - q, anom, 2 * a, 2 * b] if 2 * b < (1 << 20) else x]   # and an equal ratio
    for _ in range(3000):                                        # sums equal modulo 2^32, or with bit 31 flipped
        s = int(rng.integers(0, 1 << 40))
        t = s + int(rng.choice([G32, -G32, 5 * G32, 1 << 31, G32 - 1, 1]))
        if t < 0:
            continue
        x = [s // 2, s - s // 2, int(rng.integers(0, 3)), int(rng.integers(0, 5)), int(rng.integers(1, 9))]
        y = [t - t // 3, t // 3, int(rng.integers(0, 3)), int(rng.integers(0, 5)), int(rng.integers(1, 9))]
        A += [x, y]; B += [y, x]
    A, B = np.array(A, np.int64), np.array(B, np.int64)
    got = _predicates(api, A, B)
    want = np.array([_exact_less(list(map(int, x)), list(map(int, y))) for x, y in zip(A, B)], np.uint8)
    assert np.array_equal((got >> 5) & 1, want)
    assert np.array_equal((got >> 4) & 1, want)                 # the cross-multiplying form (bit 4) agrees
    assert want.sum() > 3000 and (want == 0).sum() > 3000


def test_k8_order_key_matches_reference_on_real_distances(T):
    """On the walk distances among the reference's truth tables (ref_algos.npz), bit 5 is the reference's operator<.  A walk
    has qul_total = its edge count >= 1 and qul_nonzero <= qul_total: the domain qe_key2's exactness argument covers
    (aasm_enum.h); tuples outside it (qul_total = 0 with a non-zero count) are not distances K8 ever holds."""
    api = T.api()
    z = np.load(os.path.join(T.GOLDEN, "ref_algos.npz"))
    a, b, want = np.ascontiguousarray(z["t1_a"]), np.ascontiguousarray(z["t1_b"]), z["t1_res"]
    got = _predicates(api, a, b)
    walk = lambda x: (x >= 0).all(1) & (x[:, 4] >= 1) & (x[:, 3] <= x[:, 4])   # noqa: E731
    real = walk(a) & walk(b)
    assert real.sum() > 500
    assert np.array_equal((got[real] >> 5) & 1, want[real] & 1)


def test_cli_on_a_wide_paf_file(T, tmp_path):
    """The binary's three files on a PAF with 10- to 13-digit coordinates equal the I/O oracle's rendering byte for byte."""
    api = T.api()
    exe = os.path.join(T.ROOT, "alignasm_amd", "alignasm")
    text = shift_paf(api.Paf.synth(20, 120, 13, dup_every=5).to_text(), 10 ** 12 + 3, 3 * G32, dlen=3 * G32)
    p = tmp_path / "wide.paf"
    p.write_bytes(text)
    want = T.io_oracle_files(text, K=64)
    r = subprocess.run([exe, str(p), "--max-paths", "64"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    for suffix, w in zip((".aln.paf", ".aln.alt.paf", ".aln.all.paf"), want):
        assert (tmp_path / ("wide" + suffix)).read_bytes() == w, suffix
    assert want[0].count(b"\n") > 100
