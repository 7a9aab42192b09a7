"""An independent restatement, in plain Python with Python ints, of the reference solver's bellman_ford()
(k_shortest_walks.hpp:91-129, with detect_cycle :94-107) and of k_shortest_walks() / kth_shortest_walk_recover() with
is_dag = false, negative_edge = true (:186): the tree step is bellman_ford over the reversed graph, the rest (:188-290) is restated
as in tests/ksw_cyclic_checker.py, whose PafDistance arithmetic and heap insert it takes.  It shares no code with the product.

bellman_ford() returns ("ok", d, prv, via), ("cycle", list) or ("invalid",) where detect_cycle would index prv[-1]; high is the queue's
high-water mark.  solve() returns ksw_cyclic_checker.solve's dict, None where the reference's BFS over tree[] would not end, or
"cycle" where bellman_ford reports one (k_shortest_walks is undefined there)."""
import heapq
from collections import deque

import numpy as np

from ksw_cyclic_checker import IDENT, MAX, _Pair, _flat, _heap_insert, add, eq, lt, sub


def bellman_ford(g, src, stats=None):           # g[v] = [(to, w, tag)]
    n = len(g)
    dis = [MAX] * n
    prv = [-1] * n
    via = [-1] * n
    dis[src] = IDENT
    q = deque([(IDENT, src)])
    high = 1
    i = 1
    while i <= n and q:
        for _ in range(len(q)):
            cur, x = q.popleft()
            if lt(dis[x], cur):                 # cur_dis > dis[x]
                continue
            for nx, w, tag in g[x]:
                cand = add(dis[x], w)
                if lt(cand, dis[nx]):
                    dis[nx] = cand
                    prv[nx] = x
                    via[nx] = tag
                    if i == n:
                        return _detect_cycle(prv, nx, n)
                    q.append((cand, nx))
                    high = max(high, len(q))
        i += 1
    if stats is not None:
        stats["high"] = high
    return ("ok", dis, prv, via)


def _detect_cycle(prv, x, n):                   # :94-107
    vis = [False] * n
    t = []
    while True:
        if x < 0:
            return ("invalid",)
        t.append(x)
        if vis[x]:
            break
        vis[x] = True
        x = prv[x]
    last = t[-1]
    t.reverse()
    while t[-1] != last:
        t.pop()
    return ("cycle", t)


def sssp(n, rowptr, col, w, src):
    """bellman_ford(g, src) on a CSR graph (w [E, 5])."""
    rowptr = [int(x) for x in rowptr]
    w = [tuple(int(x) for x in row) for row in np.asarray(w).reshape(-1, 5)]
    g = [[(int(col[e]), w[e], e) for e in range(rowptr[u], rowptr[u + 1])] for u in range(n)]
    st = {}
    r = bellman_ford(g, src, st)
    return r, st.get("high", 0)


def solve(n, rowptr, col, w, source, sink, K):
    rowptr = [int(x) for x in rowptr]
    col = [int(x) for x in col]
    w = [tuple(int(x) for x in row) for row in np.asarray(w).reshape(-1, 5)]
    g = [[(col[e], w[e]) for e in range(rowptr[u], rowptr[u + 1])] for u in range(n)]
    g_rev = [[] for _ in range(n)]              # :180-183
    for u in range(n):
        for e in range(rowptr[u], rowptr[u + 1]):
            g_rev[col[e]].append((u, w[e], e))
    r = bellman_ford(g_rev, sink)
    if r[0] != "ok":
        return "cycle"
    _, d, best, via = r
    out = {"nd": 0, "dist": _flat([]), "best": np.array(best, np.int64), "d": _flat(d), "hroot": np.full(n, -1, np.int64),
           "hcount": np.zeros(1, np.int64), "paths": [], "arena": [], "bedge": via}
    if eq(d[source], MAX):                      # :188-189
        return out
    kids = [[] for _ in range(n)]               # :191-194
    for u in range(n):
        if best[u] != -1:
            kids[best[u]].append(u)
    h = [-1] * n
    arena = []
    q, seen = [sink], {sink}                    # :198-214
    while q:
        u = q.pop(0)
        seen_p = False
        for v, wt in g[u]:
            if eq(d[v], MAX):
                continue
            c = sub(add(wt, d[v]), d[u])
            if not seen_p and v == best[u] and eq(c, IDENT):
                seen_p = True
                continue
            h[u] = _heap_insert(arena, h[u], c, (u, v))
        for p in kids[u]:
            if p in seen:
                return None
            seen.add(p)
            h[p] = h[u]
            q.append(p)
    if len(seen) != sum(1 for x in d if not eq(x, MAX)):
        return None
    distances, last = [d[source]], [-1]         # :217-249
    nodes, prev_node = [], []
    if h[source] >= 0:
        pq = []

        def emplace(dd, hp, pre):
            cur = len(nodes)
            heapq.heappush(pq, _Pair(dd, (hp, cur)))
            nodes.append(hp)
            prev_node.append(pre)

        emplace(add(d[source], arena[h[source]][1]), h[source], -1)
        while pq and len(distances) < K:
            top = heapq.heappop(pq)
            cd, (ch, cur) = top.d, top.rest
            distances.append(cd)
            last.append(cur)
            _, key, (_, v), left, right = arena[ch]
            if h[v] >= 0:
                emplace(add(cd, arena[h[v]][1]), h[v], cur)
            if left >= 0:
                emplace(sub(add(cd, arena[left][1]), key), left, prev_node[cur])
            if right >= 0:
                emplace(sub(add(cd, arena[right][1]), key), right, prev_node[cur])
    paths = []
    for k in range(len(last)):                  # :254-290
        side = []
        cur = last[k]
        while cur != -1:
            side.append(arena[nodes[cur]][2])
            cur = prev_node[cur]
        side.reverse()
        path, idx, cur = [], 0, source
        while cur != sink or idx < len(side):
            if idx < len(side) and cur == side[idx][0]:
                path += [cur, side[idx][1]]
                cur = side[idx][1]
                idx += 1
            else:
                path += [cur, best[cur]]
                cur = best[cur]
        paths.append(np.array(path, np.int64))
    out.update(nd=len(distances), dist=_flat(distances), hroot=np.array(h, np.int64), hcount=np.array([len(arena)], np.int64),
               paths=paths, arena=[[r_, *key, u, v, lf, rg] for r_, key, (u, v), lf, rg in arena])
    return out
