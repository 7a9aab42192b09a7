#!/usr/bin/env python3
"""Records tests/golden/ref_dag.npz: what the REAL reference's kShortestWalksSolver returns from topology_sort()
(k_shortest_walks.hpp:132-156) and shortest_path_dag() (:160-175) on the graphs of tests/dag_cases.py.

Run where the reference's sources lie (REF, as in oracle/Makefile):  python tests/golden/make_ref_dag.py [--ref DIR]

The recorder holds a small driver of its own (DRIVER below, in the manner of make_ref_bellman_ford.py): it builds the caller's
lists with add_edge, calls the two public functions and prints their vectors, and it defines the two globals the headers declare.
It is compiled with -DNDEBUG (the reference asserts on a cycle and then returns an empty order) against the reference's headers
where they lie, into a temporary directory that is removed afterwards; nothing of the reference is copied.  Every graph runs in a
child process of its own under a time limit, and the recorder drops none.

Per graph g: g{g}_rowptr, _col, _w (5 per edge), _meta (n, src); _order: topology_sort(g), empty for a graph with a cycle;
_d (5 per vertex) and _prv: shortest_path_dag(g, src)'s two vectors.  names[g] names the graph."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dag_cases as DC  # noqa: E402

TIME_LIMIT = 20     # seconds per graph

DRIVER = r"""
// own driver code round the reference's headers; reads one graph from stdin, writes the two functions' vectors to stdout
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <queue>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "paf_data.hpp"
#include "graph_operations.hpp"
#include "k_shortest_walks.hpp"

thread_local PafDistanceCompareMode PafDistance::cmp_mode = PafDistanceCompareMode::CALC_SUM_MODE;
bool NON_SKIP_LINKABLE = false;

using G = Graph<PafDistance>;
using Solver = kShortestWalksSolver<PafDistance, G>;

static void put(const char *tag, const std::vector<int64_t> &v) {
    printf("%s %zu", tag, v.size());
    for (int64_t x : v) printf(" %" PRId64, x);
    printf("\n");
}
static int64_t rd() { long long x; if (scanf("%lld", &x) != 1) abort(); return x; }

int main() {
    const int64_t n = rd(), E = rd(), src = rd();
    std::vector<int64_t> rowptr(n + 1), col(E), w(5 * E);
    for (auto &x : rowptr) x = rd();
    for (auto &x : col) x = rd();
    for (auto &x : w) x = rd();
    G g(n);
    for (int64_t u = 0; u < n; u++)
        for (int64_t e = rowptr[u]; e < rowptr[u + 1]; e++)
            add_edge(g, u, col[e], PafDistance(true, w[5 * e], w[5 * e + 1], w[5 * e + 2], w[5 * e + 3], w[5 * e + 4]));
    Solver s(g, PafDistance::max(), PafDistance(true), true, false);
    put("order", s.topology_sort(g));
    auto [d, prv] = s.shortest_path_dag(g, src);
    std::vector<int64_t> o;
    for (auto &x : d) { o.push_back(x.qry_score); o.push_back(x.ref_score); o.push_back(x.anom); o.push_back(x.qul_nonzero); o.push_back(x.qul_total); }
    put("d", o);
    put("prv", prv);
    printf("done\n");
    return 0;
}
"""


def default_ref():
    m = re.search(r"^REF \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    return os.environ.get("REF", m.group(1) if m else "")


def run_one(exe, g):
    text = " ".join(str(int(x)) for x in [g["n"], len(g["col"]), g["src"], *g["rowptr"], *g["col"], *g["w"].reshape(-1)])
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=TIME_LIMIT)     # a child of its own, under a time limit
    if r.returncode != 0 or not r.stdout.endswith("done\n"):
        raise RuntimeError(f"the reference's run failed: exit {r.returncode}: {r.stderr[-300:]}")
    out = {}
    for line in r.stdout.splitlines()[:-1]:
        tag, cnt, *vals = line.split()
        assert len(vals) == int(cnt), tag
        out[tag] = np.array([int(v) for v in vals], np.int64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=default_ref(), help="the reference's checkout (its src/ holds the headers)")
    a = ap.parse_args()
    src = os.path.join(a.ref, "src")
    if not os.path.isfile(os.path.join(src, "k_shortest_walks.hpp")):
        sys.exit(f"no reference sources under {src}")
    todo = DC.cases()
    out = {"n_graphs": np.array(len(todo), np.int64), "names": np.array([name for name, _ in todo])}
    done = 0
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(cpp, "w").write(DRIVER)
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-DNDEBUG", "-I" + src, "-o", exe, cpp], check=True)
        for gi, (name, g) in enumerate(todo):
            r = run_one(exe, g)
            out[f"g{gi}_rowptr"], out[f"g{gi}_col"], out[f"g{gi}_w"] = g["rowptr"], g["col"], g["w"].reshape(-1)
            out[f"g{gi}_meta"] = np.array([g["n"], g["src"]], np.int64)
            for tag in ("order", "d", "prv"):
                out[f"g{gi}_{tag}"] = r[tag]
            done += 1
            print(f"{gi:3d} {name:32s} n={g['n']:3d} E={len(g['col']):4d} src={g['src']:3d} sorted={len(r['order']):3d}")
        os.remove(exe)
    assert done == len(todo), "a graph was dropped"
    path = os.path.join(HERE, "ref_dag.npz")
    np.savez_compressed(path, **out)
    print("ref_dag.npz:", done, "graphs,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
