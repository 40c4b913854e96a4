"""The cases that hold signed re-integration (xs_tsdf_reintegrate, x-slam_amd/csrc/xs_reintegrate.hip) to a model written from the per-voxel
contract in include/xslam_amd.h and not from the kernel: a numpy statement of the rules in float32, operation by operation (the library is
built with -ffp-contract=off and divides with correct rounding, so the model is exact, not close), and a float64 twin that takes every discrete
decision (seen, the weights) from the same inputs and redoes the arithmetic in float64.  An op of the model is (sign, seen, t_value, t_grad):
the observation itself — what xs_integrate_scaled writes into a zeroed volume — is an input, synthetic in tests/test_reintegrate_cases_cpu.py
and taken from the integrate kernel's exact walk in tests/test_reintegrate_gpu.py.  Backend-neutral parts first, the device helpers after them
(the GPU tests hand torch in).  Test infrastructure.

The bound on a voxel's value after additions and removals, against the exact mean of the observations left in it (u = 2^-24, first order; ALLOW
covers the higher orders; M the largest |t| among the voxel's observations, 1 for the value channel, since a truncated distance lies in
[-1, 1]; the stored state p = P + e with P the exact mean, |P| <= M):
  Addition at weight w: fl(fl(fl(p w) + t) / (w + 1)).  float(w) and float(w + 1) are exact.  The product is off by w e + u w M, the sum
  (magnitude at most (w + 1) M) rounds by u (w + 1) M, the quotient (magnitude at most M) by u M:
      e' <= (w e + u w M + u (w + 1) M) / (w + 1) + u M <= e + 3 u M.
  Into an empty voxel (w = 0) the result is t itself: e' = 0.
  Removal at weight w >= 2: fl(fl(fl(p w) - t) / (w - 1)).  The product is off by w e + u w M, the difference (the exact one is (w - 1) Q with
  Q the mean of the others, |Q| <= M) rounds by u (w - 1) M, the quotient by u M:
      e' <= (w e + u w M + u (w - 1) M) / (w - 1) + u M = e w / (w - 1) + u M (w / (w - 1) + 2) <= 2 e + 4 u M,
  as w / (w - 1) <= 2.  The clamp of the real part to [-1, 1] moves the value towards an exact mean that lies there: it adds nothing.
  Removal at w = 1 leaves exact zeros.
  Both maps are monotone in e, and removal after addition (2 e + 10 u M) exceeds addition after removal (2 e + 7 u M): of all orders of n
  additions and m removals, all additions first is the worst.  Hence bound_u(n, m): e = 3 (n - 1), then m times e = 2 e + 4.
  Six additions and one removal: 2 * 15 + 4 = 34 u M."""
import functools

import numpy as np

U = 2.0 ** -24
ALLOW = 1.01
MAX_WEIGHT = 12
COUNT_NAMES = ("removed", "added", "emptied", "orphaned")


def bound_u(n_add, n_remove):
    """The derived constant (docstring above), in units of u M."""
    e = 3.0 * max(n_add - 1, 0)
    for _ in range(n_remove):
        e = 2.0 * e + 4.0
    return e


def bound(n_add, n_remove, M=1.0):
    return ALLOW * bound_u(n_add, n_remove) * U * float(M)


# ------------------------------------------------------------------------------------------------
# The model
def apply(state, ops, max_weight=MAX_WEIGHT, dtype=np.float32):
    """The contract on state = (value, weight, grad), arrays of one shape: returns (value, weight, grad, counts) with value and grad in dtype
    (float32: the model; float64: the twin) and counts = [removed, added, emptied, orphaned].  ops: (sign, seen, t_value, t_grad) in list order."""
    T = dtype
    v, w, g = np.array(state[0], T), np.array(state[1], np.int64), np.array(state[2], T)
    counts = [0, 0, 0, 0]
    one = T(1)
    for sign, seen, tv, tg in ops:
        assert sign in (1, -1)
        seen = np.asarray(seen, bool)
        tv, tg = np.asarray(tv).astype(T), np.asarray(tg).astype(T)
        wf = w.astype(T)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if sign > 0:
                den = (w + 1).astype(T)
                nv = (v * wf + one * tv) / den
                ng = (g * wf + one * tg) / den
                v, g = np.where(seen, nv, v), np.where(seen, ng, g)
                w = np.where(seen, np.minimum(w + 1, max_weight), w)
                counts[1] += int(seen.sum())
            else:
                take, last, none = seen & (w >= 2), seen & (w == 1), seen & (w <= 0)
                den = np.where(take, w - 1, 1).astype(T)
                nv = (v * wf - one * tv) / den
                nv = np.minimum(np.maximum(nv, -one), one)          # the real part only
                ng = (g * wf - one * tg) / den
                v = np.where(take, nv, np.where(last, T(0), v))
                g = np.where(take, ng, np.where(last, T(0), g))
                w = np.where(take, w - 1, np.where(last, 0, w))
                counts[0] += int(take.sum()) + int(last.sum())
                counts[2] += int(last.sum())
                counts[3] += int(none.sum())
    return v.astype(T), w.astype(np.int32), g.astype(T), counts


def exact_mean(obs, keep):
    """float64 mean of the observations obs[k] = (t_value, t_grad) with k in keep, per voxel (all seen)."""
    n = float(len(keep))
    return sum(np.asarray(obs[k][0], np.float64) for k in keep) / n, sum(np.asarray(obs[k][1], np.float64) for k in keep) / n


# ------------------------------------------------------------------------------------------------
# Volumes, shapes and pitches (tests/merge_cases.py: ragged, pitched, guard planes around them)
def shapes():
    import merge_cases as mc
    return [d for d, _ in mc.SHAPES]


def prior(shape, max_weight=MAX_WEIGHT):
    """A random state [Z, Y, X] x (value, weight, grad): weights 0, 1, 2 .. 9 and max_weight, values in [-1, 1] with exact +-1 and zeros."""
    X, Y, Z = shape
    rng = np.random.default_rng(7919 * X + 131 * Y + Z)
    v = rng.uniform(-1.0, 1.0, (Z, Y, X)).astype(np.float32)
    pick = rng.random((Z, Y, X))
    v[pick < 0.08] = np.float32(1.0)
    v[(pick >= 0.08) & (pick < 0.14)] = np.float32(-1.0)
    v[(pick >= 0.14) & (pick < 0.17)] = np.float32(0.0)
    g = (rng.uniform(-1.0, 1.0, (Z, Y, X)) * 1e-3).astype(np.float32)
    g[rng.random((Z, Y, X)) < 0.3] = np.float32(0.0)
    w = rng.integers(2, 10, (Z, Y, X)).astype(np.int32)
    pick = rng.random((Z, Y, X))
    w[pick < 0.2] = 0
    w[(pick >= 0.2) & (pick < 0.4)] = 1
    w[(pick >= 0.4) & (pick < 0.55)] = max_weight
    empty = w == 0
    v[empty & (pick < 0.1)] = np.float32(0.0)      # half of the empty voxels as xs_init_volume leaves them
    g[empty & (pick < 0.1)] = np.float32(0.0)
    for a in (v, w, g):
        a.setflags(write=False)
    return v, w, g


def empty(shape):
    X, Y, Z = shape
    return np.zeros((Z, Y, X), np.float32), np.zeros((Z, Y, X), np.int32), np.zeros((Z, Y, X), np.float32)


# ------------------------------------------------------------------------------------------------
# Scenes: a camera, depth images and poses for a volume of `shape`, scaled so that the volume is about 1.5 m long and the camera stands 1.4 m
# from its centre: every depth lies inside the valid range of xs_scale_depth (0.2 .. 5 m).
IMAGE_SIZES = ((32, 40), (48, 64))       # rows, cols
THRESHOLDS = (0.0, 0.05)                 # the nearest-pixel and the bilinear instance (5 cm: the tilted plane interpolates, the step does not)
DISTANCE = 1.4


def scene(shape, size_index):
    rows, cols = IMAGE_SIZES[size_index]
    vs = float(np.float32(1.537 / max(shape)))
    L = max(shape) * vs
    f = (cols / 2.0) * DISTANCE / (0.35 * L)          # the image spans about 0.7 of the volume's length at its centre
    intr = np.array([f, f * 0.97, (cols - 1) / 2.0 + 0.25, (rows - 1) / 2.0 - 0.4], np.float32)
    return dict(shape=tuple(shape), rows=rows, cols=cols, voxel_size=vs, tranc_dist=float(np.float32(min(3.5 * vs, 0.3))), intr=intr,
                threshold=THRESHOLDS[size_index])


def depth_image(rows, cols, which):
    """u16 millimetres: a tilted plane through the volume's centre, a step edge of 30 cm, 4 % zero pixels and a hole of zeros."""
    rng = np.random.default_rng(1000 + 17 * which + rows)
    u = (np.arange(cols)[None, :] - cols / 2.0) / cols
    v = (np.arange(rows)[:, None] - rows / 2.0) / rows
    tilt = (0.4, -0.3)[which % 2]
    d = DISTANCE + tilt * u + 0.25 * v
    edge = (0.6, 0.35)[which % 2]
    d = d + 0.3 * (u + 0.5 > edge)
    mm = np.round(d * 1000.0).astype(np.uint16)
    mm[rng.random((rows, cols)) < 0.04] = 0
    mm[rows // 3:rows // 3 + 4, cols // 4:cols // 4 + 5] = 0
    return mm


def _look(eye, direction):
    z = np.asarray(direction, np.float64)
    z = z / np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    Rc2v = np.stack([x, y, z], axis=1)
    Rv2c = Rc2v.T
    return Rv2c, -Rv2c @ np.asarray(eye, np.float64)


def poses(shape, voxel_size):
    """name -> (Rv2c [3, 3, 2], tv2c [3, 2]) float32.  front: the volume's centre a fifth of its length off the axis, so one side leaves the
    frustum; inside: the camera stands in the volume, part of it lies behind; oblique: along another diagonal; seeded: front's neighbour with
    imaginary parts (a complex pose); away: the volume behind the camera's back, nothing seen; back: front's opposite, the last planes nearest."""
    ext = np.array(shape, np.float64) * voxel_size
    L = ext.max()
    c = 0.5 * ext
    rng = np.random.default_rng(sum(shape))

    def pack(Rt, im=0.0):
        R, t = Rt
        Rc = np.zeros((3, 3, 2), np.float32)
        tc = np.zeros((3, 2), np.float32)
        Rc[..., 0], tc[..., 0] = R, t
        if im:
            Rc[..., 1] = im * rng.uniform(-1, 1, (3, 3))
            tc[..., 1] = im * rng.uniform(-1, 1, 3)
        return Rc, tc

    d1 = np.array([0.3, 0.2, 1.0]) / np.linalg.norm([0.3, 0.2, 1.0])
    d2 = np.array([1.0, 0.1, -0.2]) / np.linalg.norm([1.0, 0.1, -0.2])
    d3 = np.array([-0.5, 1.0, 0.4]) / np.linalg.norm([-0.5, 1.0, 0.4])
    off = np.array([0.2 * L, 0.0, 0.0])
    return {
        "front": pack(_look(c + off - DISTANCE * d1, d1)),
        "inside": pack(_look(c - 0.15 * L * d2, d2)),
        "oblique": pack(_look(c - off - DISTANCE * d3, d3)),
        "seeded": pack(_look(c + 0.9 * off - DISTANCE * d1 + 0.01, d1 + 0.01), im=1e-6),
        "away": pack(_look(c - DISTANCE * d1, -d1)),
        "back": pack(_look(c - off + DISTANCE * d1, -d1)),
    }


# op lists over a pool of observations named (image, pose): (sign, image, pose)
OP_LISTS = {
    "add": [(1, 0, "front")],
    "remove": [(-1, 0, "front")],
    "move": [(-1, 0, "front"), (1, 0, "seeded")],
    "three": [(1, 1, "inside"), (-1, 1, "inside"), (1, 0, "oblique")],
    "eight": [(1, 0, "front"), (1, 1, "inside"), (-1, 0, "front"), (1, 0, "seeded"), (-1, 1, "oblique"), (-1, 1, "inside"), (1, 0, "front"),
              (-1, 0, "away")],
    "drain": [(-1, 0, "front")] * 5 + [(-1, 1, "front")] * 3,      # weights run down to zero: emptied, then orphaned
    "fill": [(1, 0, "front"), (1, 1, "front"), (1, 0, "oblique"), (1, 1, "oblique")] * 2,   # up against max_weight
    "far": [(1, 0, "back"), (1, 1, "inside"), (-1, 0, "back"), (1, 1, "back"), (-1, 1, "oblique"), (1, 0, "seeded"), (-1, 1, "back"), (-1, 0, "back")],
}


# ------------------------------------------------------------------------------------------------
# Device side (torch is handed in by the GPU tests)
INTEGRATE_NO_TILES = 32      # XS_INTEGRATE_NO_TILES


class Scene:
    """A scene's images scaled on the device, and its observations, each computed once by the integrate kernel's exact walk into a zeroed
    volume (capi.integrate_scaled_ex with XS_INTEGRATE_NO_TILES) and then left unchanged."""

    def __init__(self, torch, capi, shape, size_index):
        self.torch, self.capi = torch, capi
        self.s = scene(shape, size_index)
        self.shape = tuple(shape)
        self.poses = poses(shape, self.s["voxel_size"])
        rows, cols = self.s["rows"], self.s["cols"]
        self.images = []
        for which in (0, 1):
            raw = torch.from_numpy(depth_image(rows, cols, which).view(np.int16)).cuda()
            scaled = torch.empty((rows, cols), dtype=torch.float32, device="cuda")
            capi.scale_depth(raw, cols * 2, rows, cols, scaled, cols * 4)
            self.images.append(scaled)
        torch.cuda.synchronize()
        self._obs = {}

    def observation(self, image, pose):
        """(seen [Z, Y, X] bool, t_value, t_grad) of image `image` at pose `pose`."""
        key = (image, pose)
        if key not in self._obs:
            torch, capi, s = self.torch, self.capi, self.s
            X, Y, Z = self.shape
            v = torch.zeros((Z * Y, X), dtype=torch.float32, device="cuda")
            w = torch.zeros((Z * Y, X), dtype=torch.int32, device="cuda")
            g = torch.zeros((Z * Y, X), dtype=torch.float32, device="cuda")
            n = torch.zeros(1, dtype=torch.int64, device="cuda")
            R, t = self.poses[pose]
            capi.integrate_scaled_ex(self.images[image], s["cols"] * 4, s["rows"], s["cols"], s["intr"], MAX_WEIGHT, list(self.shape), s["voxel_size"], R, t,
                                     s["tranc_dist"], v, w, g, X * 4, INTEGRATE_NO_TILES, threshold=s["threshold"], updated=n)
            torch.cuda.synchronize()
            wh = w.cpu().numpy().reshape(Z, Y, X)
            assert set(np.unique(wh)) <= {0, 1} and int(n.item()) == int(wh.sum())
            out = (wh == 1, v.cpu().numpy().reshape(Z, Y, X), g.cpu().numpy().reshape(Z, Y, X))
            for a in out:
                a.setflags(write=False)
            self._obs[key] = out
        return self._obs[key]

    def model_ops(self, op_list):
        return [(sign,) + self.observation(image, pose) for sign, image, pose in op_list]

    def device_ops(self, op_list):
        return [(sign, self.images[image]) + tuple(self.poses[pose]) for sign, image, pose in op_list]

    def run(self, vol, op_list, flags=0, z0=0, z1=None, counts=None, **change):
        """xs_tsdf_reintegrate of op_list on a merge_cases.DevVolume3; returns the four counts (accumulated into `counts` if given).
        `change` replaces arguments of capi.tsdf_reintegrate (the refusal test; counts_arg: what is passed as counts)."""
        torch, capi, s = self.torch, self.capi, self.s
        X, Y, Z = self.shape
        counts = torch.zeros(4, dtype=torch.int64, device="cuda") if counts is None else counts
        skip = z0 * Y * vol.pitch
        args = dict(ops=self.device_ops(op_list), scaled_step=s["cols"] * 4, rows=s["rows"], cols=s["cols"], intr=s["intr"], max_weight=MAX_WEIGHT, res=[X, Y, Z],
                    voxel_size=s["voxel_size"], tranc_dist=s["tranc_dist"], value=vol.value.addr + skip, weight=vol.weight.addr + skip,
                    grad=vol.grad.addr + skip, vol_step=vol.pitch, counts=counts, threshold=s["threshold"], z0=z0, z1=z1, flags=flags)
        if "counts_arg" in change:
            args["counts"] = change.pop("counts_arg")
        args.update(change)
        capi.tsdf_reintegrate(**args)
        torch.cuda.synchronize()
        return [int(c) for c in counts.cpu().numpy()]


def read_back(vol):
    """(value, weight, grad) [Z, Y, X] of a merge_cases.DevVolume3 as the device holds them, and whether every guard and padding word is
    still what it was."""
    Z, Y, X = vol.shape
    out, clean = [], True
    for dev, dt in ((vol.value, np.float32), (vol.weight, np.int32), (vol.grad, np.float32)):
        now = dev.buf.cpu().numpy()
        w, g = dev.pitch // 4, dev.GUARD
        off = (dev.addr - dev.buf.data_ptr()) // 4 - g * Y * w

        def inner(a):
            return a[off:off + (Z + 2 * g) * Y * w].reshape(Z + 2 * g, Y, w)[g:-g, :, :X]

        out.append(inner(now).copy().view(dt))
        rest = now.copy()
        inner(rest)[...] = inner(dev.host)
        clean = clean and np.array_equal(rest.view(np.uint32), dev.host.view(np.uint32))
    return out[0], out[1], out[2], clean


def same_words(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
