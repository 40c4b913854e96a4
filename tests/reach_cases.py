"""Shared by the clearance / reachability tests (test_reach_cpu.py, test_reach_gpu.py): the model the kernels of
xs_reach.hip are held to, built on scipy.ndimage (an exact Euclidean distance transform and a connected-component labelling, neither of
which shares anything with the kernels' three windowed passes and their word-parallel flood), a scalar brute force for tiny cases, the snap
rule in numpy and the radius derivation.  States come from view_cases.states_of.  Test infrastructure: nothing here touches the GPU."""
from collections import deque

import numpy as np
from scipy import ndimage

import view_cases as vc

UNKNOWN, FREE, OCCUPIED = vc.UNKNOWN, vc.FREE, vc.OCCUPIED
f32 = np.float32


def obstacles_of(states, unknown_blocks):
    s = np.asarray(states)
    return (s == OCCUPIED) | ((s == UNKNOWN) if unknown_blocks else np.zeros(s.shape, bool))


def clearance(states, R, unknown_blocks):
    """uint16 [Z, Y, X] = min(d^2, R^2): scipy's exact EDT with return_indices on the obstacle array padded by one layer (obstacle iff
    unknown_blocks: the nearest position outside the volume is always in that layer), squared distances from the integer indices."""
    obst = np.pad(obstacles_of(states, unknown_blocks), 1, constant_values=bool(unknown_blocks))
    if not obst.any():
        return np.full(np.asarray(states).shape, R * R, np.uint16)
    idx = ndimage.distance_transform_edt(~obst, return_distances=False, return_indices=True)
    d2 = sum((idx[k].astype(np.int64) - np.indices(obst.shape)[k]) ** 2 for k in range(3))[1:-1, 1:-1, 1:-1]
    return np.minimum(d2, R * R).astype(np.uint16)


def passable_of(states, field, r2):
    return (np.asarray(states) == FREE) & (np.asarray(field).astype(np.int64) >= int(r2))


def reached(states, field, r2, seeds):
    """bool [Z, Y, X]: the face-connected components (scipy.ndimage.label, default structure) of the passable set that hold a seed; seeds
    [N, 3] integer (x, y, z), those outside the volume or not passable contribute nothing."""
    p = passable_of(states, field, r2)
    Z, Y, X = p.shape
    lab, _ = ndimage.label(p)
    keep = set()
    for x, y, z in np.asarray(seeds, np.int64).reshape(-1, 3):
        if 0 <= x < X and 0 <= y < Y and 0 <= z < Z and lab[z, y, x]:
            keep.add(int(lab[z, y, x]))
    return np.isin(lab, sorted(keep)) & p if keep else np.zeros(p.shape, bool)


def voxel_of(points, voxel_size):
    """floor(p / voxel_size) per axis by a float32 divide: float32 [n, 3] (not yet integers: NaN and huge values stay what they are)."""
    q = np.floor(np.asarray(points, f32).reshape(-1, 3) / f32(voxel_size))
    assert q.dtype == f32
    return q


def query(points, voxel_size, mask, field, snap=0):
    """(reachable uint8 [n], clear2 uint16 [n], voxel int32 [n, 3]) by the rule of xs_reach_query over the bool mask [Z, Y, X]."""
    mask, field = np.asarray(mask, bool), np.asarray(field)
    Z, Y, X = mask.shape
    q = voxel_of(points, voxel_size)
    n = len(q)
    r, c, v = np.zeros(n, np.uint8), np.zeros(n, np.uint16), np.full((n, 3), -1, np.int32)
    for i in range(n):
        if not (q[i, 0] >= 0 and q[i, 0] < X and q[i, 1] >= 0 and q[i, 1] < Y and q[i, 2] >= 0 and q[i, 2] < Z):   # (NaN compares false)
            continue
        sx, sy, sz = (int(t) for t in q[i])
        c[i] = field[sz, sy, sx]
        if mask[sz, sy, sx]:
            r[i], v[i] = 1, (sx, sy, sz)
        elif snap > 0:
            z0, y0, x0 = max(sz - snap, 0), max(sy - snap, 0), max(sx - snap, 0)
            sub = mask[z0:sz + snap + 1, y0:sy + snap + 1, x0:sx + snap + 1]
            zz, yy, xx = np.nonzero(sub)
            if len(zz):
                zz, yy, xx = zz + z0, yy + y0, xx + x0
                d2 = (zz - sz) ** 2 + (yy - sy) ** 2 + (xx - sx) ** 2
                lin = (zz * Y + yy) * X + xx
                k = np.lexsort((lin, d2))[0]                                  # least d2, ties to the lowest linear index
                r[i], v[i], c[i] = 1, (xx[k], yy[k], zz[k]), field[zz[k], yy[k], xx[k]]
    return r, c, v


def radius_of(radius_m, voxel_size):
    """(r2, R): rv = radius_m / voxel_size in float32, r2 = max(1, ceil(rv * rv)), R the smallest integer with R^2 >= r2."""
    rv = f32(radius_m) / f32(voxel_size)
    r2 = max(1, int(np.ceil(f32(rv * rv))))
    R = 1
    while R * R < r2:
        R += 1
    return r2, R


def next_reachable_view(out4xP, reachable, min_hits):
    """view_host.hpp's rule: the largest unknown count among the reachable poses with hits >= min_hits, ties to the lower index, -1 if none."""
    best = -1
    for p, o in enumerate(np.asarray(out4xP).reshape(-1, 4)):
        if reachable[p] and int(o[2]) >= int(min_hits) and (best < 0 or int(o[0]) > int(out4xP[best][0])):
            best = p
    return best


# ---- the scalar brute force (tiny cases) ---------------------------------------------------------------------------------------------------
def brute_clearance(states, R, unknown_blocks):
    """All pairs: every voxel against every obstacle voxel, the positions outside the volume (a shell of R, at most 12, layers) included."""
    s = np.asarray(states)
    Z, Y, X = s.shape
    pad = min(R, 12)
    obst = []
    for z in range(-pad, Z + pad):
        for y in range(-pad, Y + pad):
            for x in range(-pad, X + pad):
                inside = 0 <= x < X and 0 <= y < Y and 0 <= z < Z
                if (inside and (s[z, y, x] == OCCUPIED or (unknown_blocks and s[z, y, x] == UNKNOWN))) or (not inside and unknown_blocks):
                    obst.append((x, y, z))
    o = np.array(obst, np.int64).reshape(-1, 3)
    out = np.zeros((Z, Y, X), np.uint16)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                d2 = int(((o - (x, y, z)) ** 2).sum(axis=1).min()) if len(o) else R * R
                out[z, y, x] = min(d2, R * R)
    return out


def brute_reached(states, field, r2, seeds):
    """Breadth-first search over face neighbours."""
    p = passable_of(states, field, r2)
    Z, Y, X = p.shape
    out = np.zeros(p.shape, bool)
    todo = deque()
    for x, y, z in np.asarray(seeds, np.int64).reshape(-1, 3):
        if 0 <= x < X and 0 <= y < Y and 0 <= z < Z and p[z, y, x] and not out[z, y, x]:
            out[z, y, x] = True
            todo.append((int(x), int(y), int(z)))
    while todo:
        x, y, z = todo.popleft()
        for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            a, b, c = x + dx, y + dy, z + dz
            if 0 <= a < X and 0 <= b < Y and 0 <= c < Z and p[c, b, a] and not out[c, b, a]:
                out[c, b, a] = True
                todo.append((a, b, c))
    return out


# ---- the scenes of the flood tests -----------------------------------------------------------------------------------------------------------
def random_states(res, seed, p=(0.25, 0.55, 0.2)):
    """Per-voxel random states [Z, Y, X] with probabilities (unknown, free, occupied)."""
    X, Y, Z = res
    return np.random.default_rng(seed).choice(np.array([UNKNOWN, FREE, OCCUPIED], np.uint8), size=(Z, Y, X), p=list(p))


def serpentine(res, z=5):
    """(states, path): OCCUPIED everywhere but a FREE corridor one voxel wide in plane z that runs along x on the rows y = 1, 3, 5, ... and
    turns at alternating ends: rows y = 1 and y = 3 lie in the same bricks, so the path doubles back through bricks it has left.  path: the
    corridor's voxels (x, y, z) in walking order."""
    X, Y, Z = res
    s = np.full((Z, Y, X), OCCUPIED, np.uint8)
    path = []
    rows = list(range(1, Y - 1, 2))
    for k, y in enumerate(rows):
        xs = list(range(1, X - 1)) if k % 2 == 0 else list(range(X - 2, 0, -1))
        path += [(x, y, z) for x in xs]
        if k + 1 < len(rows):
            path.append((xs[-1], y + 1, z))
    for x, y, zz in path:
        s[zz, y, x] = FREE
    return s, path


def brick_faces_crossed(path):
    return sum(1 for a, b in zip(path[:-1], path[1:]) if tuple(c >> 2 for c in a) != tuple(c >> 2 for c in b))


def jogged_corridor(res):
    """(states, start, goal): OCCUPIED everywhere but a FREE corridor of 3 x 3 voxels in cross-section along x that steps one voxel
    sideways in y half way.  On either straight piece the centre line is two voxels from the walls (field 4); at the step the nearest wall
    voxel is diagonal (field 2), so a body with r2 = 1 gets through and one with r2 = 4 does not."""
    X, Y, Z = res
    s = np.full((Z, Y, X), OCCUPIED, np.uint8)
    h = X // 2
    s[5:8, 5:8, 1:h] = FREE
    s[5:8, 6:9, h:X - 1] = FREE
    return s, (3, 6, 6), (X - 4, 7, 6)
