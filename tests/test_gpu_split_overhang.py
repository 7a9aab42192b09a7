"""GPU tier: the out-of-memory range split (test hook test_max_contigs) on the launch-form batches of
tests/test_gpu_overhang.py - records that run to or past the query's end, negative walk sums.

A module of its own, collected after tests/test_gpu_parity.py: every split releases the workspace arena, which the next
solve allocates again, and test_gpu_parity.test_cold_arena_takes_few_device_allocations bounds the device allocations the
process has made since it started."""
import pytest

import overhang_cases as O
from test_gpu_overhang import LAUNCH_BATCHES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("batch", LAUNCH_BATCHES, ids=lambda b: b[0])
def test_range_split_on_overhang_batches(T, batch):
    """Contig ranges of at most 4, solved apart and concatenated: the oracle's outputs and the whole batch's counts."""
    name, make, mode, settings = batch
    api = T.api()
    hb = make(T)
    for K, nsl in settings:
        rows = O.profile(hb, K, nsl)
        assert sum(r[1] for r in rows) > 0, rows                     # negative walks in the batch
        want = T.oracle_solve(hb, K, nsl)
        n0 = api.debug_counter("range_splits")
        split = api.solve_batch(hb, max_paths=K, non_skip_linkable=nsl, test_max_contigs=4)
        assert api.debug_counter("range_splits") > n0
        assert T.diff_outputs(want, split, stats=False) == [], (name, K, nsl)
        for k in ("n_vertices", "n_edges", "n_heap_nodes", "n_paths_found", "n_pairs"):
            assert want["stats"][k] == split["stats"][k], (name, K, nsl, k)
    O.forget()
