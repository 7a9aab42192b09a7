"""Helpers of tests/test_gpu_poison.py: the process-wide debug switch (api.debug_poison) around a solve, the guard that ends the
run on a HIP error, and the oracle's answers kept per case so that both poison bytes share one oracle run."""
import contextlib

import numpy as np
import pytest

from alignasm_amd import _abi

# 0xA5: the host emulation's byte - negative in every signed width, beyond every count, no sentinel.  0xFF: -1 in every width,
# the project's "none" - the cell that happens to look valid under 0xA5, and the reverse.
BYTES = (0xA5, 0xFF)
BYTE_IDS = ["a5", "ff"]
FAULT_WORDS = ("illegal memory access",)


def _is_fault(e):
    return (isinstance(e, RuntimeError) and getattr(e, "code", None) == _abi.AASM_E_HIP) or any(w in str(e) for w in FAULT_WORDS)


def _stop(e):
    # a stray index read from a never-written cell: a finding.  Nothing further runs on the card in this process.
    pytest.exit("poisoned run ended in a HIP error (an unwritten cell used as an index?): %s" % e, returncode=3)


@contextlib.contextmanager
def poisoned(api, byte):
    """Working memory is filled with `byte` inside the block; the switch is back at 0 after it, whatever happens."""
    prev = api.debug_poison(byte)
    try:
        assert prev == 0, "the poison switch was left on (0x%x)" % prev
        yield
    except Exception as e:                                           # (fetches and exports of a poisoned result: the same rule as for the solve)
        if _is_fault(e):
            _stop(e)
        raise
    finally:
        api.debug_poison(0)


def guarded(api, call, *args, **kw):
    """call(*args, **kw) - a solve, a graph entry, a device read, an export - under poison: AlignasmError with the HIP code, or
    any error that speaks of an illegal memory access, ends the whole run with a non-zero code; it is never retried."""
    try:
        return call(*args, **kw)
    except Exception as e:
        if _is_fault(e):
            _stop(e)
        raise


_ORACLE = {}


def oracle_outputs(T, key, hb, K, nsl=False):
    k = ("out", key, int(K), bool(nsl))
    if k not in _ORACLE:
        _ORACLE[k] = T.oracle_solve(hb, K, nsl)
    return _ORACLE[k]


def oracle_contigs(T, key, hb, K, nsl=False):
    """expect(c) for T.diff_intermediates: the oracle's intermediates of contig c, computed once per (case, K, nsl)."""
    def expect(c):
        k = ("dbg", key, int(K), bool(nsl), int(c))
        if k not in _ORACLE:
            _ORACLE[k] = T.oracle_debug(hb, c, K, nsl)
        return _ORACLE[k]
    return expect


def cached(key, make):
    if key not in _ORACLE:
        _ORACLE[key] = make()
    return _ORACLE[key]


def solve_checked(T, key, hb, K, byte, nsl=False, intermediates=True, db=None, **hooks):
    """A HIP solve of `hb` on an arena filled with `byte`: outputs and stats against the oracle, and with `intermediates` every
    intermediate as well (the cells the kernels own) -> the per-contig form flags and the counters of that solve."""
    api = T.api()
    want = oracle_outputs(T, key, hb, K, nsl)
    own = db is None
    if own:
        db = api.DeviceBatch(hb)
    try:
        with poisoned(api, byte):
            res = guarded(api, db.solve, max_paths=K, non_skip_linkable=nsl, keep_debug=intermediates, **hooks)
            try:
                got = res.fetch()
                bad = T.diff_outputs(want, got)
                assert bad == [], (hex(byte), key, hooks, bad)
                if not intermediates:
                    return None
                bad = T.diff_intermediates(hb, res.debug, K, nsl, expect=oracle_contigs(T, key, hb, K, nsl))
                assert bad == [], (hex(byte), key, hooks, bad[:6])
                C = hb.n_contigs
                return {n: res.debug(n, np.int32)[:C].copy() for n in ("gb_flag", "mw_flag", "chain_flag")} | \
                    {"counters": res.debug("counters", np.int64)[:21].copy()}
            finally:
                res.close()
    finally:
        if own:
            db.close()
