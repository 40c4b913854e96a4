"""Shared by the travel tests (test_travel_cpu.py, test_travel_gpu.py): the model the kernels of xs_travel.hip are
held to — scipy.sparse.csgraph.dijkstra over an explicitly built graph, which shares nothing with the kernels' tile relaxation in LDS —, the
path walk and the selection rule in Python integers, the float32 derivations of the limit and the bias, and a scalar brute force (heapq with
per-voxel neighbour tests) for tiny cases.  Domains are bool arrays [Z, Y, X].  Test infrastructure: nothing here touches the GPU."""
import heapq
import itertools

import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import dijkstra

NONE, MAX = 65535, 65534
f32 = np.float32
# move k = (dz + 1) 9 + (dy + 1) 3 + (dx + 1); 13 is no move
MOVES = [(k % 3 - 1, k // 3 % 3 - 1, k // 9 - 1) for k in range(27)]
COST = {1: 3, 2: 4, 3: 5}


def cost_of(o):
    return COST[sum(1 for c in o if c)]


def sub_offsets(o):
    """o with a non-empty proper subset of its non-zero components set to zero."""
    nz = [i for i in range(3) if o[i]]
    out = []
    for r in range(1, len(nz)):
        for keep in itertools.combinations(nz, r):
            out.append(tuple(o[i] if i in keep else 0 for i in range(3)))
    return out


def shifted(m, o):
    """out[v] = m[v + o], False where v + o is outside."""
    dx, dy, dz = o
    Z, Y, X = m.shape
    out = np.zeros_like(m)
    zs, zd = slice(max(0, -dz), Z - max(0, dz)), slice(max(0, dz), Z - max(0, -dz))
    ys, yd = slice(max(0, -dy), Y - max(0, dy)), slice(max(0, dy), Y - max(0, -dy))
    xs, xd = slice(max(0, -dx), X - max(0, dx)), slice(max(0, dx), X - max(0, -dx))
    out[zs, ys, xs] = m[zd, yd, xd]
    return out


def allowed(domain, o, corner_rule=True):
    """bool [Z, Y, X]: the voxels v from which the move o is allowed."""
    a = domain & shifted(domain, o)
    if corner_rule:
        for s in sub_offsets(o):
            a &= shifted(domain, s)
    return a


def seeds_in(domain, seeds):
    Z, Y, X = domain.shape
    return sorted({(int(z) * Y + int(y)) * X + int(x) for x, y, z in np.asarray(seeds, np.int64).reshape(-1, 3)
                   if 0 <= x < X and 0 <= y < Y and 0 <= z < Z and domain[z, y, x]})


def model(domain, seeds, limit=MAX, corner_rule=True):
    """uint16 [Z, Y, X]: the least cost from a seed in the domain over allowed moves, NONE above `limit` or where there is no path."""
    domain = np.asarray(domain, bool)
    Z, Y, X = domain.shape
    out = np.full(domain.shape, NONE, np.uint16)
    src = seeds_in(domain, seeds)
    if not src:
        return out
    idx = np.arange(domain.size).reshape(domain.shape)
    r, c, w = [], [], []
    for k, o in enumerate(MOVES):
        if k == 13:
            continue
        a = allowed(domain, o, corner_rule)
        frm = idx[a]
        r.append(frm)
        c.append(frm + (o[2] * Y + o[1]) * X + o[0])
        w.append(np.full(len(frm), cost_of(o), np.int32))
    g = coo_matrix((np.concatenate(w), (np.concatenate(r), np.concatenate(c))), shape=(domain.size, domain.size)).tocsr()
    d = dijkstra(g, directed=True, indices=src, min_only=True).reshape(domain.shape)
    ok = np.isfinite(d) & (d <= limit)
    out[ok] = d[ok].astype(np.uint16)
    return out


def move_allowed(domain, v, o):
    """The scalar statement of the rule: v = (x, y, z) in the domain, v + o and every v + o' in it."""
    Z, Y, X = domain.shape

    def inside(p):
        return 0 <= p[0] < X and 0 <= p[1] < Y and 0 <= p[2] < Z and bool(domain[p[2], p[1], p[0]])
    return inside(v) and all(inside((v[0] + s[0], v[1] + s[1], v[2] + s[2])) for s in [o] + sub_offsets(o))


def brute(domain, seeds, limit=MAX):
    """Dijkstra by hand: a heap of (cost, voxel), the 26 moves tested one voxel at a time."""
    domain = np.asarray(domain, bool)
    Z, Y, X = domain.shape
    out = np.full(domain.shape, NONE, np.uint16)
    best, heap = {}, []
    for s in seeds_in(domain, seeds):
        v = (s % X, s // X % Y, s // (X * Y))
        best[v] = 0
        heap.append((0, v))
    heapq.heapify(heap)
    while heap:
        c, v = heapq.heappop(heap)
        if c > best[v]:
            continue
        for k, o in enumerate(MOVES):
            if k == 13 or not move_allowed(domain, v, o):
                continue
            u, cu = (v[0] + o[0], v[1] + o[1], v[2] + o[2]), c + cost_of(o)
            if cu <= limit and cu < best.get(u, 1 << 60):
                best[u] = cu
                heapq.heappush(heap, (cu, u))
    for (x, y, z), c in best.items():
        out[z, y, x] = c
    return out


def walk(travel, domain, target):
    """The path from `target` down the field: a list of (x, y, z), target first and the seed last; [] when travel[target] is NONE or the
    target is outside.  Each step takes the allowed move with travel[v + o] + w(o) = travel[v] that has the lowest index k."""
    Z, Y, X = travel.shape
    x, y, z = (int(t) for t in target)
    if not (0 <= x < X and 0 <= y < Y and 0 <= z < Z) or int(travel[z, y, x]) == NONE:
        return []
    path = [(x, y, z)]
    while int(travel[z, y, x]) != 0:
        here = int(travel[z, y, x])
        for k, o in enumerate(MOVES):
            if k != 13 and move_allowed(domain, (x, y, z), o) and int(travel[z + o[2], y + o[1], x + o[0]]) + cost_of(o) == here:
                x, y, z = x + o[0], y + o[1], z + o[2]
                break
        else:
            raise AssertionError(("not a fixpoint: no move explains", (x, y, z), here))
        path.append((x, y, z))
    return path


def travel_limit(max_travel_m, voxel_size):
    """view_host.hpp's travel_limit: 65534 for max_travel_m <= 0 or not finite, otherwise min(65534, floor(3 m / voxel)) in float32."""
    m = f32(max_travel_m)
    if not (m > 0) or not np.isfinite(m):
        return MAX
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        u = np.floor(f32(f32(3) * m) / f32(voxel_size))
    return int(u) if u < MAX else MAX


def travel_bias(bias_m, voxel_size):
    """view_host.hpp's travel_bias: max(1, ceil(3 bias / voxel)) in float32."""
    u = np.ceil(f32(f32(3) * f32(bias_m)) / f32(voxel_size))
    return max(1, int(u))


def next_view_by_travel(out4xP, travel, min_hits, bias3):
    """view_host.hpp's rule in Python integers: among the poses with a cost and hits >= min_hits the largest unknown / (travel + bias3) by
    cross-multiplication, ties to the lower index, -1 if none."""
    best = -1
    o = [[int(v) for v in row] for row in np.asarray(out4xP).reshape(-1, 4)]
    t = [int(v) for v in np.asarray(travel).reshape(-1)]
    for p in range(len(o)):
        if t[p] == NONE or o[p][2] < int(min_hits):
            continue
        if best < 0 or o[p][0] * (t[best] + int(bias3)) > o[best][0] * (t[p] + int(bias3)):
            best = p
    return best
