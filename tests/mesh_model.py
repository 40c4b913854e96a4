"""Independent numpy statement of xs_extract_mesh's vertex set (include/xslam_amd.h, surface mesh): which edges carry a vertex, where it
sits (float32, the point export's expression) and its imaginary part (complex128).  It needs no case table: a vertex is a sign-changing
edge of at least one live cube."""
import numpy as np


def live_cubes(value, weight, z0, z1, zs0=0, min_weight=1):
    """bool [z1 - z0, Y - 1, X - 1]: cube (x, y, z0 + k) is live.  value / weight: [planes, Y, X] starting at stored plane zs0."""
    v = value[z0 - zs0:z1 + 1 - zs0]
    w = weight[z0 - zs0:z1 + 1 - zs0]
    ok = (w >= min_weight) & (v < np.float32(0.99))
    neg = v < 0
    all_ok = np.ones((z1 - z0, v.shape[1] - 1, v.shape[2] - 1), bool)
    n_neg = np.zeros(all_ok.shape, np.int32)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                sl = (slice(dz, dz + z1 - z0), slice(dy, dy + v.shape[1] - 1), slice(dx, dx + v.shape[2] - 1))
                all_ok &= ok[sl]
                n_neg += neg[sl]
    return all_ok & (n_neg > 0) & (n_neg < 8)


def vertices(value, weight, res, voxel_size, z0=0, z1=None, zs0=0, min_weight=1, grad=None):
    """(keys uint64 [V] ascending, positions float32 [V, 3], imaginary parts float64 [V, 3] or None)."""
    X, Y, Z = (int(r) for r in res)
    z1 = Z - 1 if z1 is None else z1
    live = live_cubes(value, weight, z0, z1, zs0, min_weight)
    P = z1 - z0 + 1                                  # planes of lower endpoints: [z0, z1]
    livep = np.zeros((P + 1, Y + 1, X + 1), bool)    # livep[k + 1, y + 1, x + 1] = cube (x, y, z0 + k) live
    livep[1:P, 1:Y, 1:X] = live
    v = value[z0 - zs0:z1 + 1 - zs0].astype(np.float32)
    neg = v < 0
    vs = np.float32(voxel_size)
    keys, pos, ims = [], [], []
    for ax in range(3):
        d = [0, 0, 0]
        d[ax] = 1
        dx, dy, dz = d
        # edge (x, y, z) -> (x, y, z) + e_ax, for all lower endpoints in planes [z0, z1]
        cz, cy, cx = np.meshgrid(np.arange(P), np.arange(Y), np.arange(X), indexing="ij")
        inside = (cx + dx < X) & (cy + dy < Y) & (cz + dz < P)
        cz, cy, cx = cz[inside], cy[inside], cx[inside]
        change = neg[cz, cy, cx] != neg[cz + dz, cy + dy, cx + dx]
        others = [k for k in range(3) if k != ax]
        adj = np.zeros(cz.shape, bool)
        for o1 in (0, 1):
            for o2 in (0, 1):
                o = [0, 0, 0]
                o[others[0]], o[others[1]] = o1, o2
                adj |= livep[cz - o[2] + 1, cy - o[1] + 1, cx - o[0] + 1]
        sel = change & adj
        cz, cy, cx = cz[sel], cy[sel], cx[sel]
        F = v[cz, cy, cx]
        Fn = v[cz + dz, cy + dy, cx + dx]
        gz = cz + z0
        V = [(cx.astype(np.float32) + np.float32(0.5)) * vs, (cy.astype(np.float32) + np.float32(0.5)) * vs,
             (gz.astype(np.float32) + np.float32(0.5)) * vs]
        p = [V[0].copy(), V[1].copy(), V[2].copy()]
        p[ax] = V[ax] - (F / (Fn - F)) * vs
        keys.append(((gz.astype(np.uint64) * Y + cy.astype(np.uint64)) * X + cx.astype(np.uint64)) * 3 + ax)
        pos.append(np.stack(p, 1).astype(np.float32))
        if grad is not None:
            g = grad[z0 - zs0:z1 + 1 - zs0].astype(np.float64)
            Fc = F.astype(np.float64) + 1j * g[cz, cy, cx]
            Fnc = Fn.astype(np.float64) + 1j * g[cz + dz, cy + dy, cx + dx]
            im = np.zeros((len(cz), 3))
            im[:, ax] = (V[ax].astype(np.float64) - (Fc / (Fnc - Fc)) * float(vs)).imag
            ims.append(im)
    keys = np.concatenate(keys)
    order = np.argsort(keys, kind="stable")
    return keys[order], np.concatenate(pos)[order], (np.concatenate(ims)[order] if grad is not None else None)
