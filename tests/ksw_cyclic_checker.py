"""An independent restatement, in plain Python with Python ints, of what the reference's solver computes for
k_shortest_walks(source, sink, k) and kth_shortest_walk_recover() on a graph that may hold cycles (is_dag = false,
negative_edge = false):

  PafDistance        paf_data.hpp:142-188    the order (CALC_SUM mode), operator== and the arithmetic
  dijkstra()         k_shortest_walks.hpp:69-87 on the reversed graph built as :180-183
  heaps, k pops      :191-249, a heap node's pointer replaced by its allocation index (the monotonic allocator's order)
  recovery           :254-290

It shares no code with the product or the oracle.  solve() returns the dict shape of aasm_testlib.generic_run (nd, dist, best,
d, hroot, hcount, paths), so ksw_cases.compare takes it, and the heap arena beside it.  The tree step is a parameter: "dijkstra"
(the branch restated here) or "dag" (:132-175, to check the restatement against the recorded DAG runs)."""
import heapq

import numpy as np

MAX = (-1, -1, -1, -1, 0)
IDENT = (0, 0, 0, 0, 0)


# ---- PafDistance (paf_data.hpp:142-188) ---------------------------------------------------------------------------------
def eq(a, b):                                   # :163-168
    tot = a[4] if a[4] else 1
    rtot = b[4] if b[4] else 1
    return a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[3] * rtot == b[3] * tot


def lt(a, b):                                   # :142-159, CALC_SUM_MODE
    if eq(a, MAX):
        return False
    if eq(b, MAX):
        return True
    if a[0] + a[1] != b[0] + b[1]:
        return a[0] + a[1] < b[0] + b[1]
    if a[2] != b[2]:
        return a[2] < b[2]
    tot = a[4] if a[4] else 1
    rtot = b[4] if b[4] else 1
    return a[3] * rtot > b[3] * tot


def add(a, b):                                  # :178-183
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2], a[3] + b[3], a[4] + b[4])


def sub(a, b):                                  # :184-188
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2], a[3] - b[3], a[4] - b[4])


class _Pair:
    """An entry of a std::priority_queue with std::greater: (Distance, then the rest as a tuple of ints)."""
    __slots__ = ("d", "rest")

    def __init__(self, d, rest):
        self.d, self.rest = d, rest

    def __lt__(self, o):
        if lt(self.d, o.d):
            return True
        if lt(o.d, self.d):
            return False
        return self.rest < o.rest


class Overflow(Exception):
    """dijkstra() made more pushes than the caller allows (the reference would go on)."""


# ---- the shortest-path tree ---------------------------------------------------------------------------------------------
def dijkstra(g, src, push_limit=None):          # :69-87; g[v] = [(to, w, tag)]; returns d, prv, tag of the relaxing entry, pushes
    d = [MAX] * len(g)
    prv = [-1] * len(g)
    via = [-1] * len(g)
    d[src] = IDENT
    heap = [_Pair(IDENT, src)]
    pushes = 1
    while heap:
        top = heapq.heappop(heap)
        dv, v = top.d, top.rest
        if not eq(dv, d[v]):
            continue
        for to, w, tag in g[v]:
            cand = add(dv, w)
            if lt(cand, d[to]):
                d[to] = cand
                pushes += 1
                if push_limit is not None and pushes > push_limit:
                    raise Overflow()
                heapq.heappush(heap, _Pair(cand, to))
                prv[to] = v
                via[to] = tag
    return d, prv, via, pushes


def shortest_path_dag(g, s):                    # :132-175
    n = len(g)
    in_deg = [0] * n
    for u in range(n):
        for v, _, _ in g[u]:
            in_deg[v] += 1
    q = [u for u in range(n) if not in_deg[u]]
    order = []
    while q:
        u = q.pop(0)
        order.append(u)
        for v, _, _ in g[u]:
            in_deg[v] -= 1
            if in_deg[v] == 0:
                q.append(v)
    assert len(order) == n, "cycle in a DAG"
    d = [MAX] * n
    prv = [-1] * n
    via = [-1] * n
    d[s] = IDENT
    for v in order:
        if eq(d[v], MAX):
            continue
        for to, w, tag in g[v]:
            cand = add(d[v], w)
            if lt(cand, d[to]):
                d[to] = cand
                prv[to] = v
                via[to] = tag
    return d, prv, via, 0


# ---- k_shortest_walks (:179-251) and the recovery (:254-290) ------------------------------------------------------------------
def _heap_insert(arena, a, k, v):               # leftist_heap.hpp:29-40; a node is [rank, key, value, left, right], a pointer its index
    if a < 0 or not lt(arena[a][1], k):
        arena.append([1, k, v, a, -1])
        return len(arena) - 1
    l, r = arena[a][3], _heap_insert(arena, arena[a][4], k, v)
    if l < 0 or arena[l][0] < arena[r][0]:
        l, r = r, l
    arena.append([arena[r][0] + 1 if r >= 0 else 0, arena[a][1], arena[a][2], l, r])
    return len(arena) - 1


def solve(n, rowptr, col, w, source, sink, K, tree="dijkstra", push_limit=None):
    """The solver on one graph (CSR, w [E, 5]).  Returns None where the reference's own BFS over tree[] would not end (best[] is
    no tree into the sink); raises Overflow past push_limit.  dist, d are flat int64 arrays (object arrays beyond int64)."""
    rowptr = [int(x) for x in rowptr]
    col = [int(x) for x in col]
    w = [tuple(int(x) for x in row) for row in np.asarray(w).reshape(-1, 5)]
    g = [[(col[e], w[e]) for e in range(rowptr[u], rowptr[u + 1])] for u in range(n)]
    g_rev = [[] for _ in range(n)]              # :180-183
    for u in range(n):
        for e in range(rowptr[u], rowptr[u + 1]):
            g_rev[col[e]].append((u, w[e], e))
    d, best, via, pushes = (dijkstra(g_rev, sink, push_limit) if tree == "dijkstra" else shortest_path_dag(g_rev, sink))
    out = {"nd": 0, "dist": _flat([]), "best": np.array(best, np.int64), "d": _flat(d), "hroot": np.full(n, -1, np.int64),
           "hcount": np.zeros(1, np.int64), "paths": [], "arena": [], "pushes": pushes, "bedge": via}
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
            if p in seen:                       # the reference goes round for ever
                return None
            seen.add(p)
            h[p] = h[u]
            q.append(p)
    if len(seen) != sum(1 for x in d if not eq(x, MAX)):
        return None                             # a vertex with a distance whose best[] chain misses the sink: recovery does not end
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
               paths=paths, arena=[[r, *key, u, v, lf, rg] for r, key, (u, v), lf, rg in arena])
    return out


def _flat(ds):
    vals = [x for t in ds for x in t]
    if all(-(1 << 63) <= x < (1 << 63) for x in vals):
        return np.array(vals, np.int64).reshape(-1)
    return np.array(vals, object).reshape(-1)
