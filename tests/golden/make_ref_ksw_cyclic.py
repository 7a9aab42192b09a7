#!/usr/bin/env python3
"""Records tests/golden/ref_ksw_cyclic.npz: what the REAL reference's kShortestWalksSolver computes with is_dag = false,
negative_edge = false (k_shortest_walks.hpp:65,185) on the graphs of tests/ksw_cyclic_cases.py - the hand-made ones and 40 random
cyclic graphs, ten of each kind.

Run where the reference's sources lie (REF, as in oracle/Makefile):  python tests/golden/make_ref_ksw_cyclic.py [--ref DIR]

The recorder holds a small driver of its own (DRIVER below, in the manner of oracle/ref_harness.cpp): a never-reusing bump
operator new, so that pointer order is allocation order - the order the product's arena index restates -, `private` lifted
round the one include so the solver's d, best, h and alloc can be read, and the two globals the headers declare.  It is
compiled against the reference's headers where they lie, into a temporary directory that is removed afterwards; nothing of the
reference is copied.  Every graph runs in a child process of its own under a time limit, and the recorder drops none.

Per graph g the file holds what ref_algos.npz holds for its DAGs, as far as it exists without a topological order: g{g}_rowptr,
_col, _w (5 per edge), _meta (n, source, sink, K), _dist (5 per walk), _best, _d (5 per vertex), _hroot (arena index, -1 = null),
_hcount, _path_len, _paths ((u, v) pairs), and _arena ({rank, key[5], u, v, left, right} per heap node); names[g] names it."""
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
import ksw_cyclic_cases as CC  # noqa: E402

TIME_LIMIT = 20     # seconds per graph

DRIVER = r"""
// own driver code round the reference's headers; reads one graph from stdin, writes the solver's state to stdout
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <new>
#include <queue>
#include <string>
#include <tuple>
#include <utility>
#include <vector>
#include <sys/mman.h>

namespace {
char *g_arena = nullptr; size_t g_cap = 0, g_top = 0;
}
void *operator new(size_t n) {
    if (!g_arena) {
        g_cap = (size_t)8 << 30;
        g_arena = (char *)mmap(nullptr, g_cap, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (g_arena == MAP_FAILED) abort();
    }
    const size_t a = (g_top + 15) & ~(size_t)15;
    if (a + n > g_cap) throw std::bad_alloc();
    g_top = a + n;
    return g_arena + a;
}
void *operator new[](size_t n) { return operator new(n); }
void operator delete(void *) noexcept {}
void operator delete[](void *) noexcept {}
void operator delete(void *, size_t) noexcept {}
void operator delete[](void *, size_t) noexcept {}

#include "paf_data.hpp"
#include "graph_operations.hpp"
#define private public
#include "k_shortest_walks.hpp"
#undef private

thread_local PafDistanceCompareMode PafDistance::cmp_mode = PafDistanceCompareMode::CALC_SUM_MODE;
bool NON_SKIP_LINKABLE = false;

using G = Graph<PafDistance>;
using Solver = kShortestWalksSolver<PafDistance, G>;

static void put(const char *tag, const std::vector<int64_t> &v) {
    printf("%s %zu", tag, v.size());
    for (int64_t x : v) printf(" %" PRId64, x);
    printf("\n");
}
static void add5(std::vector<int64_t> &o, const PafDistance &d) {
    o.push_back(d.qry_score); o.push_back(d.ref_score); o.push_back(d.anom); o.push_back(d.qul_nonzero); o.push_back(d.qul_total);
}
static int64_t rd() { long long x; if (scanf("%lld", &x) != 1) abort(); return x; }

int main() {
    const int64_t n = rd(), E = rd(), source = rd(), sink = rd(), K = rd();
    std::vector<int64_t> rowptr(n + 1), col(E), w(5 * E);
    for (auto &x : rowptr) x = rd();
    for (auto &x : col) x = rd();
    for (auto &x : w) x = rd();
    G g(n);
    for (int64_t u = 0; u < n; u++)
        for (int64_t e = rowptr[u]; e < rowptr[u + 1]; e++)
            add_edge(g, u, col[e], PafDistance(true, w[5 * e], w[5 * e + 1], w[5 * e + 2], w[5 * e + 3], w[5 * e + 4]));
    Solver s(g, PafDistance::max(), PafDistance(true), false, false);
    auto dist = s.k_shortest_walks(source, sink, K);
    std::vector<int64_t> o;
    for (auto &x : dist) add5(o, x);
    put("dist", o);
    put("best", s.best);
    o.clear();
    for (auto &x : s.d) add5(o, x);
    put("d", o);
    std::map<const Solver::heap_t *, int64_t> idx;
    for (auto &nd : s.alloc) { const int64_t i = (int64_t)idx.size(); idx[&nd] = i; }
    auto at = [&](const Solver::heap_t *p) -> int64_t { return p ? idx.at(p) : -1; };
    o.clear();
    if (!dist.empty()) for (auto *p : s.h) o.push_back(at(p));
    else o.assign(n, -1);
    put("hroot", o);
    put("hcount", {(int64_t)s.alloc.size()});
    o.clear();
    for (auto &nd : s.alloc) {
        o.push_back(nd.node_rank); add5(o, nd.key); o.push_back(nd.value.first); o.push_back(nd.value.second);
        o.push_back(at(nd.left)); o.push_back(at(nd.right));
    }
    put("arena", o);
    std::vector<int64_t> len, uv;
    for (int64_t k = 0; k < (int64_t)dist.size(); k++) {
        auto p = s.kth_shortest_walk_recover(source, sink, k, false);
        len.push_back(2 * (int64_t)p.size());
        for (auto &[a, b, ww] : p) { uv.push_back(a); uv.push_back(b); }
    }
    put("path_len", len);
    put("paths", uv);
    printf("done\n");
    return 0;
}
"""


def default_ref():
    m = re.search(r"^REF \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    return os.environ.get("REF", m.group(1) if m else "")


def cases():
    """(name, graph, K): K = 60 everywhere (so that one batch at k = 60 can be checked), but 400 for every tenth random graph."""
    out = [(name, g, 60) for name, g in CC.hand_graphs()]
    for i, g in enumerate(CC.random_graphs(20241, 40)):
        out.append((f"random_{g['kind']}_{i}", g, 60 if i % 10 else 400))
    return out


def run_one(exe, g, K):
    text = " ".join(str(int(x)) for x in [g["n"], len(g["col"]), g["src"], g["sink"], K, *g["rowptr"], *g["col"], *g["w"].reshape(-1)])
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
    todo = cases()
    out = {"n_graphs": np.array(len(todo), np.int64), "names": np.array([name for name, _, _ in todo])}
    done = 0
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(cpp, "w").write(DRIVER)
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-DNDEBUG", "-I" + src, "-o", exe, cpp], check=True)
        for gi, (name, g, K) in enumerate(todo):
            r = run_one(exe, g, K)
            out[f"g{gi}_rowptr"], out[f"g{gi}_col"], out[f"g{gi}_w"] = g["rowptr"], g["col"], g["w"].reshape(-1)
            out[f"g{gi}_meta"] = np.array([g["n"], g["src"], g["sink"], K], np.int64)
            for tag in ("dist", "best", "d", "hroot", "hcount", "arena", "path_len", "paths"):
                out[f"g{gi}_{tag}"] = r[tag]
            done += 1
            print(f"{gi:3d} {name:32s} n={g['n']:3d} E={len(g['col']):3d} K={K:3d} walks={len(r['dist']) // 5:3d} heap={int(r['hcount'][0])}")
        os.remove(exe)
    assert done == len(todo), "a graph was dropped"
    path = os.path.join(HERE, "ref_ksw_cyclic.npz")
    np.savez_compressed(path, **out)
    print("ref_ksw_cyclic.npz:", done, "graphs,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
