"""Shared by the view-scoring tests (test_score_views_cpu.py, test_score_views_gpu.py): the float32 numpy model of
xs_score_views' arithmetic contract (include/xslam_amd.h), a triple-loop restatement of it in plain Python for tiny cases, the volumes a
state array stands for, the known-answer scene and the pose sets.  Test infrastructure: nothing here touches the GPU."""
import numpy as np

UNKNOWN, FREE, OCCUPIED = 0, 1, 2
f32 = np.float32
INTR = (525.0, 525.0, 319.5, 239.5)
ROWS, COLS = 480, 640


def states_of(value, weight, min_weight=1):
    """The observation grid's rule on arrays of any shape: uint8 states."""
    mw = max(int(min_weight), 1)
    v, w = np.asarray(value, f32), np.asarray(weight, np.int32)
    return np.where(w < mw, UNKNOWN, np.where(v < 0, OCCUPIED, FREE)).astype(np.uint8)


def volumes_of(states):
    """(value float32, weight int32) of a state array: UNKNOWN -> weight 0, value 0; FREE -> weight 1, value 1.0; OCCUPIED -> weight 1,
    value -0.5."""
    s = np.asarray(states)
    value = np.where(s == FREE, f32(1.0), np.where(s == OCCUPIED, f32(-0.5), f32(0.0))).astype(f32)
    weight = (s != UNKNOWN).astype(np.int32)
    return value, weight


def sample_depths(t_near, t_far, step):
    """t_k = t_near + float(k) * step for k = 0, 1, ... while t_k < t_far (float32; no running sum)."""
    t_near, t_far, step = f32(t_near), f32(t_far), f32(step)
    out = []
    k = 0
    while True:
        t = f32(t_near + f32(f32(k) * step))
        if not t < t_far:
            break
        out.append(t)
        k += 1
        assert k <= 1 << 16
    return np.array(out, f32)


def model(states, R, t, intr, rows, cols, voxel_size, rays=(80, 60), t_near=0.2, t_far=5.0, step=None):
    """The contract, vectorised over the rays of one pose: states uint8 [Z, Y, X], R [3, 3] and t [3] camera to volume.  Returns uint32 [4]
    = {unknown, free, hits, frontier}.  Every operation is one float32 operation, in the contract's order."""
    states = np.asarray(states)
    Z, Y, X = states.shape
    R, t = np.asarray(R, f32), np.asarray(t, f32)
    fx, fy, cx, cy = (f32(v) for v in intr)
    vs = f32(voxel_size)
    rx, ry = int(rays[0]), int(rays[1])
    ts = sample_depths(t_near, t_far, vs if step is None else step)
    i = np.arange(rx, dtype=f32)[None, :].repeat(ry, 0).reshape(-1)
    j = np.arange(ry, dtype=f32)[:, None].repeat(rx, 1).reshape(-1)
    u = (i + f32(0.5)) * (f32(cols) / f32(rx))
    v = (j + f32(0.5)) * (f32(rows) / f32(ry))
    dx, dy = (u - cx) / fx, (v - cy) / fy
    assert dx.dtype == f32 and dy.dtype == f32
    d = [(R[c, 0] * dx + R[c, 1] * dy) + R[c, 2] for c in range(3)]
    n = rx * ry
    alive = np.ones(n, bool)
    prev_free = np.zeros(n, bool)
    out = np.zeros(4, np.uint64)
    for tk in ts:
        p = [t[c] + tk * d[c] for c in range(3)]
        q = [np.floor(p[c] / vs) for c in range(3)]
        assert q[0].dtype == f32
        inside = alive & (q[0] >= 0) & (q[0] < X) & (q[1] >= 0) & (q[1] < Y) & (q[2] >= 0) & (q[2] < Z)   # (NaN compares false)
        idx = np.flatnonzero(inside)
        s = states[q[2][idx].astype(np.int64), q[1][idx].astype(np.int64), q[0][idx].astype(np.int64)]
        unk, fre, occ = idx[s == UNKNOWN], idx[s == FREE], idx[s == OCCUPIED]
        out[0] += len(unk)
        out[3] += int(prev_free[unk].sum())
        out[1] += len(fre)
        out[2] += len(occ)
        prev_free[unk] = False
        prev_free[fre] = True
        alive[occ] = False
    return out.astype(np.uint32)


def model_poses(states, Rs, ts, *args, **kw):
    return np.stack([model(states, R, t, *args, **kw) for R, t in zip(Rs, ts)])


def restatement(states, R, t, intr, rows, cols, voxel_size, rays, t_near, t_far, step):
    """The same contract ray by ray and sample by sample in plain Python loops, scalars only (for tiny cases)."""
    Z, Y, X = np.asarray(states).shape
    fx, fy, cx, cy = (f32(v) for v in intr)
    vs, t_near, t_far, step = f32(voxel_size), f32(t_near), f32(t_far), f32(step)
    R, t = np.asarray(R, f32), np.asarray(t, f32)
    out = [0, 0, 0, 0]
    for j in range(rays[1]):
        for i in range(rays[0]):
            u = f32(f32(f32(i) + f32(0.5)) * f32(f32(cols) / f32(rays[0])))
            v = f32(f32(f32(j) + f32(0.5)) * f32(f32(rows) / f32(rays[1])))
            dx, dy = f32(f32(u - cx) / fx), f32(f32(v - cy) / fy)
            d = [f32(f32(f32(R[c, 0] * dx) + f32(R[c, 1] * dy)) + R[c, 2]) for c in range(3)]
            prev_free = False
            k = 0
            while True:
                tk = f32(t_near + f32(f32(k) * step))
                if not tk < t_far:
                    break
                k += 1
                vox = [int(np.floor(f32(f32(t[c] + f32(tk * d[c])) / vs))) for c in range(3)]
                if not (0 <= vox[0] < X and 0 <= vox[1] < Y and 0 <= vox[2] < Z):
                    continue
                s = int(states[vox[2], vox[1], vox[0]])
                if s == OCCUPIED:
                    out[2] += 1
                    break
                if s == FREE:
                    out[1] += 1
                    prev_free = True
                else:
                    out[0] += 1
                    out[3] += int(prev_free)
                    prev_free = False
    return np.array(out, np.uint32)


def next_best_view(out4xP, min_hits):
    """view_host.hpp's rule: the largest unknown count among the poses with hits >= min_hits, ties to the lower index, -1 if none."""
    best = -1
    for p, o in enumerate(np.asarray(out4xP).reshape(-1, 4)):
        if int(o[2]) >= int(min_hits) and (best < 0 or int(o[0]) > int(out4xP[best][0])):
            best = p
    return best


# ---- the known-answer scene (the issue's table) -------------------------------------------------------------------------------------------
KNOWN_N = 64
KNOWN_VOXEL = f32(3.0 / 64.0)
KNOWN_T = np.array([1.0, 1.5, 0.6], f32)
KNOWN_ANGLES = (0.0, -0.5, 0.5, 1.0, float(np.pi))
KNOWN_COUNTS = np.array([[34740, 162300, 2880, 1440], [0, 155220, 2220, 0], [121800, 103260, 1380, 3420], [172860, 46260, 0, 4800],
                         [0, 43200, 0, 0]], np.uint32)
KNOWN_MIN_HITS, KNOWN_BEST = 1200, 2


def known_states():
    """[z, y, x]: x >= 32 UNKNOWN; x < 32: FREE for z < 56, OCCUPIED for 56 <= z < 60, UNKNOWN above."""
    s = np.zeros((KNOWN_N,) * 3, np.uint8)
    s[:56, :, :32] = FREE
    s[56:60, :, :32] = OCCUPIED
    return s


def rot_y(a):
    """Rotation about y by a, computed in float64 and rounded to float32."""
    c, s = np.cos(np.float64(a)), np.sin(np.float64(a))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float64).astype(f32)


def known_poses():
    return np.stack([rot_y(a) for a in KNOWN_ANGLES]), np.stack([KNOWN_T] * len(KNOWN_ANGLES))


# ---- the kernel-versus-model case ---------------------------------------------------------------------------------------------------------
CASE_RES = (20, 18, 13)          # X, Y, Z: partial bricks on all three axes
CASE_VOXEL, CASE_NEAR, CASE_FAR, CASE_STEP = f32(0.05), f32(0.2), f32(2.0), f32(0.05)


def random_volume(res, seed):
    """Per-voxel random (value, weight), dense [Z, Y, X]: weights from {0, 1, 2, 5}, values from {-0.5, 0, 1, -0.0, a tiny negative}."""
    rng = np.random.default_rng(seed)
    X, Y, Z = res
    weight = rng.choice(np.array([0, 1, 2, 5], np.int32), size=(Z, Y, X)).astype(np.int32)
    value = rng.choice(np.array([-0.5, 0.0, 1.0, -0.0, -1e-30], f32), size=(Z, Y, X)).astype(f32)
    return value, weight


def random_rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(f32)


def case_poses(n_random=24, seed=11):
    """(R [P, 3, 3], t [P, 3], names) for a volume of CASE_RES x CASE_VOXEL (1.0 x 0.9 x 0.65 m): inside the volume, outside looking in,
    looking away (all zeros), 20 m off, identity with t on exact multiples of the voxel size (samples on voxel faces), random rigid poses."""
    rng = np.random.default_rng(seed)
    eye = np.eye(3, dtype=f32)
    R = [rot_y(0.3), eye, rot_y(np.pi), eye, eye]
    t = [np.array([0.5, 0.45, 0.1], f32), np.array([0.5, 0.45, -0.5], f32), np.array([0.5, 0.45, -0.5], f32), np.array([20.0, 0.4, 0.3], f32),
         np.array([10, 9, 0], f32) * CASE_VOXEL]
    names = ["inside", "outside_looking_in", "looking_away", "far_off", "on_voxel_faces"]
    for k in range(n_random):
        R.append(random_rotation(rng))
        t.append((rng.uniform(-0.3, 1.2, size=3) * np.array([1.0, 0.9, 0.65])).astype(f32))
        names.append(f"random{k}")
    return np.stack(R), np.stack(t), names


def as_c2v32(R, t):
    """[P, 4, 4, 2] float32 camera2volume matrices (zero imaginary parts) from R [P, 3, 3], t [P, 3]."""
    P = len(R)
    m = np.zeros((P, 4, 4, 2), f32)
    m[:, :3, :3, 0] = R
    m[:, :3, 3, 0] = t
    m[:, 3, 3, 0] = 1.0
    return m
