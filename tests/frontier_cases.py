"""Shared by the frontier tests (test_frontier_cpu.py, test_frontier_gpu.py): the model the kernels of
xs_frontier.hip are held to — the frontier by padded boolean shifts of the states, the clusters by scipy.ndimage.label with the full
3 x 3 x 3 structure run per cell block and made canonical by scipy.ndimage.minimum over the global linear index, the records by
np.bincount / np.minimum.at (none of which shares anything with the kernels' word-parallel mask, their min-label fixpoint in LDS or their
atomics) —, a scalar brute force for tiny cases, and numpy twins of the host algebra of x-slam_amd/host/view_host.hpp.  States come from
view_cases / reach_cases.  Test infrastructure: nothing here touches the GPU."""
from collections import deque

import numpy as np
from scipy import ndimage

import view_cases as vc

UNKNOWN, FREE, OCCUPIED = vc.UNKNOWN, vc.FREE, vc.OCCUPIED
NONE = 0xFFFFFFFF
f32 = np.float32


def frontier(states):
    """bool [Z, Y, X]: FREE with at least one UNKNOWN face neighbour inside the volume (the padding is not UNKNOWN)."""
    s = np.asarray(states)
    unk = np.pad(s == UNKNOWN, 1, constant_values=False)
    near = np.zeros(s.shape, bool)
    for axis in range(3):
        for shift in (0, 2):
            sl = [slice(1, -1)] * 3
            sl[axis] = slice(shift, shift + s.shape[axis])
            near |= unk[tuple(sl)]
    return (s == FREE) & near


def linear_index(shape):
    Z, Y, X = shape
    return np.arange(Z * Y * X, dtype=np.int64).reshape(Z, Y, X)


def labels(mask, cell):
    """uint32 [Z, Y, X]: the lowest linear index (z Y + y) X + x of each voxel's cluster, NONE off the mask.  Clusters: the 26-connected
    components of the mask inside each cell (cubes of `cell` voxels aligned to the origin; 0: one cell)."""
    mask = np.asarray(mask, bool)
    Z, Y, X = mask.shape
    lin = linear_index(mask.shape)
    out = np.full(mask.shape, NONE, np.uint32)
    c = cell if cell else max(X, Y, Z)
    for z0 in range(0, Z, c):
        for y0 in range(0, Y, c):
            for x0 in range(0, X, c):
                sl = (slice(z0, z0 + c), slice(y0, y0 + c), slice(x0, x0 + c))
                lab, n = ndimage.label(mask[sl], structure=np.ones((3, 3, 3), bool))
                if n == 0:
                    continue
                low = np.asarray(ndimage.minimum(lin[sl], lab, index=np.arange(1, n + 1))).astype(np.int64)
                sub = out[sl]
                sub[lab > 0] = low[lab[lab > 0] - 1].astype(np.uint32)
    return out


def records(lab):
    """uint64 [n, 8] in ascending label order: {label, count, sum x, sum y, sum z, min x | y << 16 | z << 32, max likewise, 0}."""
    lab = np.asarray(lab)
    Z, Y, X = lab.shape
    zz, yy, xx = np.nonzero(lab != NONE)
    if len(zz) == 0:
        return np.zeros((0, 8), np.uint64)
    roots, inv = np.unique(lab[zz, yy, xx], return_inverse=True)
    n = len(roots)
    out = np.zeros((n, 8), np.uint64)
    out[:, 0] = roots
    out[:, 1] = np.bincount(inv, minlength=n)
    lo, hi = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for k, coord in enumerate((xx, yy, zz)):
        out[:, 2 + k] = np.bincount(inv, weights=coord.astype(np.float64), minlength=n).astype(np.uint64)   # (exact: far below 2^53)
        a, b = np.full(n, 1 << 40, np.int64), np.full(n, -1, np.int64)
        np.minimum.at(a, inv, coord)
        np.maximum.at(b, inv, coord)
        lo |= a.astype(np.uint64) << np.uint64(16 * k)
        hi |= b.astype(np.uint64) << np.uint64(16 * k)
    out[:, 5], out[:, 6] = lo, hi
    return out


def model(states, cell):
    """(mask bool, labels uint32, records uint64 [n, 8]) of a state array."""
    m = frontier(states)
    lab = labels(m, cell)
    return m, lab, records(lab)


# ---- the scalar brute force (tiny cases) -----------------------------------------------------------------------------------------------------
def brute(states, cell):
    """The same three results by per-voxel neighbour tests and a breadth-first search over the 26 neighbours within the cell."""
    s = np.asarray(states)
    Z, Y, X = s.shape
    m = np.zeros(s.shape, bool)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                if s[z, y, x] != FREE:
                    continue
                for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                    a, b, c = x + dx, y + dy, z + dz
                    if 0 <= a < X and 0 <= b < Y and 0 <= c < Z and s[c, b, a] == UNKNOWN:
                        m[z, y, x] = True
    cell_of = (lambda v: 0) if not cell else (lambda v: v // cell)
    lab = np.full(s.shape, NONE, np.uint32)
    recs = []
    for z in range(Z):                                                          # ascending linear index: the first voxel met is the root
        for y in range(Y):
            for x in range(X):
                if not m[z, y, x] or lab[z, y, x] != NONE:
                    continue
                root = (z * Y + y) * X + x
                lab[z, y, x] = root
                todo, members = deque([(x, y, z)]), []
                while todo:
                    a, b, c = todo.popleft()
                    members.append((a, b, c))
                    for dz in (-1, 0, 1):
                        for dy in (-1, 0, 1):
                            for dx in (-1, 0, 1):
                                p, q, r = a + dx, b + dy, c + dz
                                if not (0 <= p < X and 0 <= q < Y and 0 <= r < Z) or not m[r, q, p] or lab[r, q, p] != NONE:
                                    continue
                                if (cell_of(p), cell_of(q), cell_of(r)) != (cell_of(a), cell_of(b), cell_of(c)):
                                    continue
                                lab[r, q, p] = root
                                todo.append((p, q, r))
                xs, ys, zs = zip(*members)
                recs.append([root, len(members), sum(xs), sum(ys), sum(zs), min(xs) | min(ys) << 16 | min(zs) << 32, max(xs) | max(ys) << 16 | max(zs) << 32, 0])
    return m, lab, np.array(recs, np.uint64).reshape(-1, 8)


# ---- the host algebra (view_host.hpp) in numpy -------------------------------------------------------------------------------------------
def centroid(rec, voxel_size):
    """float32 [3]: ((float32)(sum / count in float64) + 0.5) * voxel_size per axis."""
    q = (np.asarray(rec[2:5], np.float64) / np.float64(rec[1])).astype(f32)
    return ((q + f32(0.5)) * f32(voxel_size)).astype(f32)


def unpack_box(word):
    return tuple(int((int(word) >> s) & 0xFFFF) for s in (0, 16, 32))


def halton(index, base):
    f, r = 1.0, 0.0
    while index > 0:
        f /= base
        r += f * (index % base)
        index //= base
    return r


def direction(j):
    """float64 [3]: the unit vector of the Halton pair (bases 2 and 3, index j + 1) with z = 1 - 2 u, phi = 2 pi v."""
    u, v = halton(j + 1, 2), halton(j + 1, 3)
    z = 1.0 - 2.0 * u
    r = np.sqrt(max(0.0, 1.0 - z * z))
    return np.array([r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v), z])


def voxel_centre(v, voxel_size):
    return (np.asarray(v).astype(f32) + f32(0.5)) * f32(voxel_size)


def look_at(pos, target, hint_down, hint_side, hint_cos=0.99):
    """float64 [3, 3] (columns x, y, z of the camera in volume coordinates), or None: the rule of view_host.hpp's look_at."""
    z = np.asarray(target, np.float64) - np.asarray(pos, np.float64)
    n = np.linalg.norm(z)
    if not n > 0:
        return None
    z = z / n
    for h in (hint_down, hint_side):
        h = np.asarray(h, np.float64)
        hn = np.linalg.norm(h)
        if not hn > 0 or abs(h @ z) / hn > hint_cos:
            continue
        x = np.cross(h, z)
        x /= np.linalg.norm(x)
        return np.stack([x, np.cross(z, x), z], axis=1)
    return None
