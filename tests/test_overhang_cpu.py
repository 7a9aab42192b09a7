"""CPU tier: records that run to or past the query's end (tests/overhang_cases.py) - negative dest edges, negative walk sums,
contigs whose K walks cross zero - through the product's kernel bodies (1-lane host emulation), the oracle and, where it was
built, the reference's own solve_ctg_read() prefix.  (The sorted-runs queue of K8 does not run in the emulation:
tests/test_gpu_overhang.py is where it meets these inputs.)"""
import numpy as np
import pytest

import overhang_cases as O
from test_fuzz import make_batch

SETTINGS = ((10000, False), (3, True))                               # test_fuzz._run's
WIDE_L = 10 ** 8                                                     # at L = 400 under 0.1 % of the walks are negative: large coordinates matter


def _fuzz(seeds, L):
    for seed in seeds:
        for style in (0, 1, 2):
            base = make_batch(seed, 6, 25, L, style)
            for mode in O.MODES:
                yield (seed, style, mode), O.overhang(base, mode, seed)


def _tally(seen, hb, K, nsl):
    for found, neg, lo, hi in O.profile(hb, K, nsl):
        seen["walks"] += found
        seen["negative"] += neg
        seen["crossing"] += 1 if (found and lo < 0 <= hi) else 0


# ---- a. fuzz: emulation against oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [400, WIDE_L], ids=["L400", "L1e8"])
def test_overhang_fuzz_emulation_vs_oracle(T, L):
    seen = dict(walks=0, negative=0, crossing=0, paths=0)
    for key, hb in _fuzz(range(24), L):
        for K, nsl in SETTINGS:
            want = T.oracle_solve(hb, K, nsl)
            got = T.emul_solve(hb, K, nsl)
            assert T.diff_outputs(want, got) == [], (key, K, nsl)
            if K == 10000:
                assert T.diff_intermediates(hb, T.emul_debug, K, nsl, expect=O.expect(hb, K, nsl)) == [], (key, K, nsl)
            _tally(seen, hb, K, nsl)
            seen["paths"] += want["stats"]["n_paths_found"]
        O.forget()
    print("L = %d: %s" % (L, seen))
    assert seen["paths"] > 1000
    if L == WIDE_L:                                                  # what the inputs are meant to contain, on the oracle alone
        assert seen["negative"] >= 0.30 * seen["walks"], seen
        assert seen["crossing"] >= 40, seen                          # contig-solves with walks on both sides of zero
    else:
        assert seen["negative"] > 0, seen


# ---- b. the emulation's other forms ---------------------------------------------------------------------------------------------
HOOKS = [dict(chain="all"), dict(chain="none"), dict(graph_launches=True), dict(heap_waves="all"), dict(sequential_select=True),
         dict(test_small_root_ring=True)]


@pytest.mark.parametrize("hooks", HOOKS, ids=lambda h: "_".join("%s=%s" % kv for kv in h.items()))
def test_overhang_fuzz_emulation_hooks(T, hooks):
    seen = dict(walks=0, negative=0, crossing=0)
    for key, hb in _fuzz(range(6), WIDE_L):
        for K, nsl in SETTINGS:
            want = _oracle_out(T, key, hb, K, nsl)
            assert T.diff_outputs(want, T.emul_solve(hb, K, nsl, **hooks)) == [], (key, K, nsl, hooks)
            if K == 10000:
                assert T.diff_intermediates(hb, T.emul_debug, K, nsl, expect=_oracle_dbg(T, key, hb, K, nsl)) == [], (key, K, nsl, hooks)
    for key, hb in _fuzz(range(6), WIDE_L):
        for K, nsl in SETTINGS:
            for c in range(hb.n_contigs):
                o = _oracle_dbg(T, key, hb, K, nsl)(c)
                if o is not None:
                    s = o["kd_qry"] + o["kd_ref"]
                    seen["walks"] += len(s); seen["negative"] += int((s < 0).sum()); seen["crossing"] += 1 if s.min() < 0 <= s.max() else 0
    assert seen["negative"] >= 0.30 * seen["walks"] and seen["crossing"] >= 10, seen      # (a quarter of a.'s seeds, a quarter of its 40)


_KEPT = {}                                                           # the six hook cases share one oracle run per (batch, K, nsl)


def _oracle_out(T, key, hb, K, nsl):
    k = ("out", key, K, nsl)
    if k not in _KEPT:
        _KEPT[k] = T.oracle_solve(hb, K, nsl)
    return _KEPT[k]


def _oracle_dbg(T, key, hb, K, nsl):
    off = hb.arrays["ctg_rec_off"]

    def expect(c):
        if off[c + 1] - off[c] <= 1:
            return None
        k = ("dbg", key, K, nsl, c)
        if k not in _KEPT:
            _KEPT[k] = T.oracle_debug(hb, c, K, nsl)
        return _KEPT[k]
    return expect


# ---- c. the live reference --------------------------------------------------------------------------------------------------------
def _diff_reference(T, hb, contigs, nsl):
    """oracle_debug vs the reference's solve_ctg_read() prefix over all PREFIX_NAMES -> (mismatches, #distances, #negative distances, smallest edge weight)."""
    bad, nd, nneg, wmin = [], 0, 0, 1 << 62
    off = hb.arrays["ctg_rec_off"]
    for c in contigs:
        if off[c + 1] - off[c] <= 1:
            continue
        r = T.ref_prefix_debug(hb, c, nsl=nsl)
        o = T.oracle_debug(hb, c, 10000, nsl)
        assert "vtx_index_mismatch" not in r
        bad += [(c, n) for n in T.PREFIX_NAMES if not np.array_equal(o[n], r[n])]
        nd += len(r["kd_qry"]); nneg += int((r["kd_qry"] + r["kd_ref"] < 0).sum())
        wmin = min(wmin, int(r["csr_w_qry"].min()))
    return bad, nd, nneg, wmin


def _need_reference(T):
    if T.ref_prefix(True) is None:
        pytest.skip("oracle/_ref/libaasm_ref_prefix*.so not built (no /root/reference on this box and no prebuilt .so)")


@pytest.mark.ref
@pytest.mark.parametrize("mode", O.MODES)
def test_oracle_matches_reference_prefix_on_overhang_fuzz(T, mode):
    """12 fuzz contigs per mode (two batches of six), both NON_SKIP_LINKABLE settings, at large coordinates."""
    _need_reference(T)
    nd = nneg = 0
    wmin = []
    for seed, style in ((50, 0), (51, 2)):
        hb = O.overhang(make_batch(seed, 6, 30, WIDE_L, style), mode, seed)
        for nsl in (False, True):
            bad, a, b, w = _diff_reference(T, hb, range(6), nsl)
            assert bad == [], (mode, seed, nsl, bad[:4])
            nd += a; nneg += b; wmin.append(w)
    assert nd > 1000
    if mode == "zero":
        assert nneg == nd
    elif mode == "longest":
        assert set(wmin) == {-2}                                     # one dest edge per contig below zero, by 2
    elif mode == "touch":
        assert set(wmin) == {0} and nneg == 0                        # the in-domain edge
    else:
        assert 0 < nneg < nd, (mode, nd, nneg)


@pytest.mark.ref
@pytest.mark.parametrize("case", [(1, 300, 5, False, 3), (1, 200, 31, True, 0)], ids=["sparse_dup3", "dense"])
def test_oracle_matches_reference_prefix_on_centred_contigs(T, case):
    """Contigs whose 10 000 walks cross zero half-way: the reference's own distances do, and the oracle's equal them."""
    _need_reference(T)
    nc, nr, seed, dense, dup = case
    hb = O.centre(T.synth(nc, nr, seed, dense=dense, dup_every=dup), 10000)
    assert hb.skipped == []
    bad, nd, nneg, _ = _diff_reference(T, hb, range(nc), False)
    assert bad == []
    assert nd >= 4 and nd // 4 <= nneg <= nd - nd // 4, (nd, nneg)
