#!/usr/bin/env python3
"""Records tests/golden/ref_bellman_ford.npz: what the REAL reference's kShortestWalksSolver computes with negative weights on the
graphs of tests/bf_cases.py - bellman_ford() itself (k_shortest_walks.hpp:91-129), the solver with is_dag = false, negative_edge =
true (:186), and on the negative DAGs the solver with is_dag = true.

Run where the reference's sources lie (REF, as in oracle/Makefile):  python tests/golden/make_ref_bellman_ford.py [--ref DIR]

The recorder holds a small driver of its own (DRIVER below, in the manner of make_ref_ksw_cyclic.py): a never-reusing bump operator
new, so that pointer order is allocation order, `private` lifted round the one include, and the two globals the headers declare.  It
is compiled with -DNDEBUG (the reference asserts on a negative cycle and then returns it) against the reference's headers where they
lie, into a temporary directory that is removed afterwards; nothing of the reference is copied.  Every graph runs in a child process
of its own under a time limit, and the recorder drops none.

Per graph g: g{g}_rowptr, _col, _w (5 per edge), _meta (n, source, sink, K); of bellman_ford(g, source): _bf_status (0, or 1 for a
negative cycle), _bf_d (5 per vertex; max where there is a cycle, the reference returns no vector), _bf_prv, _bf_cycle;
_rev_status: the same status of bellman_ford(g_rev, sink), the call k_shortest_walks makes.  Where that is 0 the solver's run in
ref_ksw_cyclic.npz's fields: _dist, _best, _d, _hroot, _hcount, _path_len, _paths, _arena; k_shortest_walks is not called where it is
1 - the reference would index an empty vector.  The graphs of kind neg_dag hold the same fields once more as _dag_*, from the solver
with is_dag = true.  names[g] names the graph."""
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
import bf_cases as BC  # noqa: E402

TIME_LIMIT = 20     # seconds per graph
KSW_TAGS = ("dist", "best", "d", "hroot", "hcount", "arena", "path_len", "paths")

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

static void put(const std::string &tag, const std::vector<int64_t> &v) {
    printf("%s %zu", tag.c_str(), v.size());
    for (int64_t x : v) printf(" %" PRId64, x);
    printf("\n");
}
static void add5(std::vector<int64_t> &o, const PafDistance &d) {
    o.push_back(d.qry_score); o.push_back(d.ref_score); o.push_back(d.anom); o.push_back(d.qul_nonzero); o.push_back(d.qul_total);
}
static int64_t rd() { long long x; if (scanf("%lld", &x) != 1) abort(); return x; }

// the solver's state after k_shortest_walks, every walk recovered
static void ksw(const G &g, int64_t n, int64_t source, int64_t sink, int64_t K, bool is_dag, const std::string &pre) {
    Solver s(g, PafDistance::max(), PafDistance(true), is_dag, true);
    auto dist = s.k_shortest_walks(source, sink, K);
    std::vector<int64_t> o;
    for (auto &x : dist) add5(o, x);
    put(pre + "dist", o);
    put(pre + "best", s.best);
    o.clear();
    for (auto &x : s.d) add5(o, x);
    put(pre + "d", o);
    std::map<const Solver::heap_t *, int64_t> idx;
    for (auto &nd : s.alloc) { const int64_t i = (int64_t)idx.size(); idx[&nd] = i; }
    auto at = [&](const Solver::heap_t *p) -> int64_t { return p ? idx.at(p) : -1; };
    o.clear();
    if (!dist.empty()) for (auto *p : s.h) o.push_back(at(p));
    else o.assign(n, -1);
    put(pre + "hroot", o);
    put(pre + "hcount", {(int64_t)s.alloc.size()});
    o.clear();
    for (auto &nd : s.alloc) {
        o.push_back(nd.node_rank); add5(o, nd.key); o.push_back(nd.value.first); o.push_back(nd.value.second);
        o.push_back(at(nd.left)); o.push_back(at(nd.right));
    }
    put(pre + "arena", o);
    std::vector<int64_t> len, uv;
    for (int64_t k = 0; k < (int64_t)dist.size(); k++) {
        auto p = s.kth_shortest_walk_recover(source, sink, k, false);
        len.push_back(2 * (int64_t)p.size());
        for (auto &[a, b, ww] : p) { uv.push_back(a); uv.push_back(b); }
    }
    put(pre + "path_len", len);
    put(pre + "paths", uv);
}

int main() {
    const int64_t n = rd(), E = rd(), source = rd(), sink = rd(), K = rd(), dag = rd();
    std::vector<int64_t> rowptr(n + 1), col(E), w(5 * E);
    for (auto &x : rowptr) x = rd();
    for (auto &x : col) x = rd();
    for (auto &x : w) x = rd();
    G g(n), g_rev(n);
    for (int64_t u = 0; u < n; u++)
        for (int64_t e = rowptr[u]; e < rowptr[u + 1]; e++)
            add_edge(g, u, col[e], PafDistance(true, w[5 * e], w[5 * e + 1], w[5 * e + 2], w[5 * e + 3], w[5 * e + 4]));
    for (int64_t u = 0; u < n; u++)
        for (auto &[v, ww] : g[u]) g_rev[v].push_back({u, ww});
    {
        Solver s(g, PafDistance::max(), PafDistance(true), false, true);
        auto [dis, second] = s.bellman_ford(g, source);
        const bool cyc = dis.empty();
        std::vector<int64_t> o;
        if (cyc) for (int64_t v = 0; v < n; v++) add5(o, PafDistance::max());
        else for (auto &x : dis) add5(o, x);
        put("bf_status", {cyc ? 1 : 0});
        put("bf_d", o);
        put("bf_prv", cyc ? std::vector<int64_t>(n, -1) : second);
        put("bf_cycle", cyc ? second : std::vector<int64_t>());
    }
    bool rev_cyc;
    {
        Solver s(g, PafDistance::max(), PafDistance(true), false, true);
        rev_cyc = s.bellman_ford(g_rev, sink).first.empty();
        put("rev_status", {rev_cyc ? 1 : 0});
    }
    if (!rev_cyc) ksw(g, n, source, sink, K, false, "");
    if (dag) ksw(g, n, source, sink, K, true, "dag_");
    printf("done\n");
    return 0;
}
"""


def default_ref():
    m = re.search(r"^REF \?= *(\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
    return os.environ.get("REF", m.group(1) if m else "")


def run_one(exe, g, K, dag):
    text = " ".join(str(int(x)) for x in [g["n"], len(g["col"]), g["src"], g["sink"], K, int(dag), *g["rowptr"], *g["col"], *g["w"].reshape(-1)])
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
    todo = BC.cases()
    out = {"n_graphs": np.array(len(todo), np.int64), "names": np.array([name for name, _, _ in todo])}
    done = 0
    with tempfile.TemporaryDirectory() as tmp:
        cpp, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
        open(cpp, "w").write(DRIVER)
        subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-DNDEBUG", "-I" + src, "-o", exe, cpp], check=True)
        for gi, (name, g, K) in enumerate(todo):
            # detect_cycle would index prv[-1]: such a graph cannot be recorded (there is none among the cases)
            assert BC.checker_bf(g)[0]["status"] in (0, 1), name
            dag = g.get("kind") == "neg_dag"
            r = run_one(exe, g, K, dag)
            out[f"g{gi}_rowptr"], out[f"g{gi}_col"], out[f"g{gi}_w"] = g["rowptr"], g["col"], g["w"].reshape(-1)
            out[f"g{gi}_meta"] = np.array([g["n"], g["src"], g["sink"], K], np.int64)
            for tag in ("bf_status", "bf_d", "bf_prv", "bf_cycle", "rev_status"):
                out[f"g{gi}_{tag}"] = r[tag]
            for pre in ([""] if not r["rev_status"][0] else []) + (["dag_"] if dag else []):
                for tag in KSW_TAGS:
                    out[f"g{gi}_{pre}{tag}"] = r[pre + tag]
            done += 1
            walks = len(r["dist"]) // 5 if "dist" in r else -1
            print(f"{gi:3d} {name:36s} n={g['n']:3d} E={len(g['col']):3d} K={K:3d} bf={int(r['bf_status'][0])} rev={int(r['rev_status'][0])} walks={walks:3d}")
        os.remove(exe)
    assert done == len(todo), "a graph was dropped"
    path = os.path.join(HERE, "ref_bellman_ford.npz")
    np.savez_compressed(path, **out)
    print("ref_bellman_ford.npz:", done, "graphs,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
