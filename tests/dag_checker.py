"""An independent restatement, in plain Python with Python ints, of the reference solver's topology_sort()
(k_shortest_walks.hpp:132-156) and shortest_path_dag() (:160-175), with PafDistance's order (paf_data.hpp:136-183, CALC_SUM mode)
written out here.  It shares no code with the product and serves the graphs that nobody recorded.

topology_sort(g) returns the Kahn order with a FIFO queue, or [] for a graph with a cycle (the reference built with NDEBUG);
shortest_path_dag(g, s) returns (d, prv): on a cycle the order is empty and nothing is relaxed."""
from collections import deque

import numpy as np

MAX = (-1, -1, -1, -1, 0)       # PafDistance::max(): PafDistance(false, -1, -1, -1, -1), qul_total defaulted to 0
IDENT = (0, 0, 0, 0, 0)         # PafDistance(true)


def eq(a, b):                   # operator== (:163-168)
    tot, rtot = a[4] or 1, b[4] or 1
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] * rtot == b[3] * tot


def lt(a, b):                   # operator< (:142-159), CALC_SUM_MODE
    if eq(a, MAX):
        return False
    if eq(b, MAX):
        return True
    if a[0] + a[1] != b[0] + b[1]:
        return a[0] + a[1] < b[0] + b[1]
    if a[2] != b[2]:
        return a[2] < b[2]
    tot, rtot = a[4] or 1, b[4] or 1
    return a[3] * rtot > b[3] * tot


def add(a, b):                  # operator+ (:178-183)
    return tuple(x + y for x, y in zip(a, b))


def topology_sort(g):           # g[u] = [(v, w)]
    n = len(g)
    in_deg = [0] * n
    for u in range(n):
        for v, _ in g[u]:
            in_deg[v] += 1
    q = deque(u for u in range(n) if not in_deg[u])
    out = []
    for _ in range(n):
        if not q:
            return []           # "Cycle occured in DAG": cleared and returned
        u = q.popleft()
        out.append(u)
        for v, _ in g[u]:
            in_deg[v] -= 1
            if in_deg[v] == 0:
                q.append(v)
    return out


def shortest_path_dag(g, s):
    n = len(g)
    d = [MAX] * n
    prv = [-1] * n
    d[s] = IDENT
    for v in topology_sort(g):
        if eq(d[v], MAX):
            continue
        for to, w in g[v]:
            cand = add(d[v], w)
            if lt(cand, d[to]):     # d_[to] > d_[v] + w
                d[to] = cand
                prv[to] = v
    return d, prv


def lists(n, rowptr, col, w):
    rowptr = [int(x) for x in rowptr]
    w = [tuple(int(x) for x in row) for row in np.asarray(w).reshape(-1, 5)]
    return [[(int(col[e]), w[e]) for e in range(rowptr[u], rowptr[u + 1])] for u in range(n)]


def solve(n, rowptr, col, w, src):
    """The recorded shape: {status, order (-1 everywhere on a cycle), d (5 per vertex), prv}."""
    g = lists(n, rowptr, col, w)
    order = topology_sort(g)
    d, prv = shortest_path_dag(g, src)
    return {"status": 0 if len(order) == n else 1, "order": np.array(order if len(order) == n else [-1] * n, np.int64),
            "d": np.array([x for t in d for x in t], np.int64), "prv": np.array(prv, np.int64)}
