"""The binding's functions that take no instance and no GPU: the host library's CPU entry points, the pose candidates, the configuration
text, the process-wide stream, and the named tuples the instance methods return."""
import collections
import ctypes as C

import numpy as np

from .pipeline_abi import _f32p, _f64p, _i32p, _lib


def yaml_text(params: dict) -> str:
    """Flat YAML in the reference's format (ICL_traj2.yaml) from a dict of its keys."""
    out = []
    for k, v in params.items():
        if isinstance(v, bool):
            v = "true" if v else "false"
        elif isinstance(v, float):
            v = repr(float(np.float32(v))) if abs(v) < 1e-3 and v != 0 else repr(v)
        out.append(f"{k}: {v}")
    return "\n".join(out) + "\n"


HDC_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "sqrt": 4, "abs": 5, "exp": 6, "log": 7, "sin": 8, "cos": 9, "pow": 10, "f1": 11,
           "conj": 12, "norm": 13, "cmp": 14}


def host_double_complex(op, a, b=None):
    """Elementwise host DoubleComplex op over [n, 4] float32 arrays (CPU; no GPU involved)."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 4)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 4)
    out = np.empty_like(a)
    rc = _lib.xs_host_double_complex_table(HDC_OPS[op], a.shape[0], a.ctypes.data_as(_f32p), b.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
    if rc != 0:
        raise ValueError("bad op")
    return out


def host_complex(op_code, a, b=None):
    """Elementwise complex<float> op of csrc/xs_complex.h compiled for the host, over [n, 2] float32 arrays (CPU)."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 2)
    b = a if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1, 2)
    out = np.empty_like(a)
    rc = _lib.xs_host_complex_table(int(op_code), a.shape[0], a.ctypes.data_as(_f32p), b.ctypes.data_as(_f32p), out.ctypes.data_as(_f32p))
    if rc != 0:
        raise ValueError("bad op")
    return out


def host_newton_seeded_poses(c2v):
    """The 21 dual-complex seeded poses of a Newton pass for camera2volume c2v [4, 4, 2]: (R [21, 3, 3, 4], t [21, 3, 4]) float32, pair
    (a, b), a <= b, row-major (CPU; no GPU involved)."""
    m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32)
    R, t = np.zeros((21, 3, 3, 4), np.float32), np.zeros((21, 3, 4), np.float32)
    _lib.xs_host_newton_seeded_poses(m.ctypes.data_as(_f32p), R.ctypes.data_as(_f32p), t.ctypes.data_as(_f32p))
    return R, t


def host_newton_step(s29, damping, c2v):
    """One Newton step on the 29 scaled sums of pose_hessian: (taken, c2v [4, 4, 2]); not taken (c2v unchanged) when count < 6 or
    H + damping diag(H) is not positive definite (CPU)."""
    s = np.ascontiguousarray(s29, dtype=np.float64).reshape(29)
    m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32).copy()
    rc = _lib.xs_host_newton_step(s.ctypes.data_as(_f64p), float(damping), m.ctypes.data_as(_f32p))
    return rc == 0, m.reshape(4, 4, 2)


def _real44(m):
    """A real 4 x 4 float64 from a 4 x 4 (real) or 4 x 4 x 2 (re, im: the real parts) pose."""
    a = np.asarray(m, dtype=np.float64)
    if a.shape == (4, 4, 2):
        a = a[..., 0]
    return np.ascontiguousarray(a.reshape(4, 4))


def merge_affine(T, dst_voxel_size, src_voxel_size):
    """xform12 of capi.tsdf_merge (float32 [12]: 3 x 3 row-major, then 3 offsets) from T (real 4 x 4: a point of the destination map's volume
    frame, in metres, to the source map's) and the two voxel sizes: float64 throughout, one rounding at the end (CPU).  ValueError for an
    input that is not finite or a voxel size that is not positive."""
    t = _real44(T)
    out = np.zeros(12, np.float32)
    if _lib.xs_host_merge_affine(t.ctypes.data_as(_f64p), float(dst_voxel_size), float(src_voxel_size), out.ctypes.data_as(_f32p)) != 0:
        raise ValueError("merge_affine: an input is not finite, or a voxel size is not positive")
    return out


def map_transform(c2v_this, c2v_other):
    """T = c2v_other c2v_this^-1 (real 4 x 4 float64) from the real parts of two camera-to-volume poses of one camera frame: the frame's pose in
    this map and, by relocalize_global there, in the other map give the T that merge_map takes (CPU)."""
    a, b = _real44(c2v_this), _real44(c2v_other)
    out = np.zeros((4, 4), np.float64)
    _lib.xs_host_map_transform(a.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p), out.ctypes.data_as(_f64p))
    return out


def align_seeded_maps(T, vs_this, vs_other):
    """The six complex-seeded index maps of one alignment pass (float32 [6, 12, 2]: xform12's entries as (re, im)) from T (real 4 x 4, as
    merge_affine takes it): T_k = (I + i h G_k) T through merge_affine's formula, three translations then three rotations.  The real parts
    are merge_affine's bit for bit (CPU).  ValueError: merge_affine's refusals."""
    t = _real44(T)
    out = np.zeros((6, 12, 2), np.float32)
    if _lib.xs_host_align_seeded_maps(t.ctypes.data_as(_f64p), float(vs_this), float(vs_other), out.ctypes.data_as(_f32p)) != 0:
        raise ValueError("align_seeded_maps: an input is not finite, or a voxel size is not positive")
    return out


def align_step(s29, damping, T):
    """One damped Gauss-Newton step on the 29 scaled sums of an alignment pass: (taken, T [4, 4] float64) with T <- exp(delta) T; not taken
    (T unchanged) when count < 6 or A + damping diag(A) is not positive definite (CPU)."""
    s = np.ascontiguousarray(s29, dtype=np.float64).reshape(29)
    t = _real44(T).copy()
    rc = _lib.xs_host_align_step(s.ctypes.data_as(_f64p), float(damping), t.ctypes.data_as(_f64p))
    return rc == 0, t


def register_step(s29, damping, T):
    """One damped Gauss-Newton step on the 29 sums of capi.register_terms as they stand (no scaling): (taken, T [4, 4] float64) with
    T <- exp(delta) T, delta = (translation, rotation); not taken (T unchanged) when count < 6 or A + damping diag(A) is not positive
    definite (CPU)."""
    s = np.ascontiguousarray(s29, dtype=np.float64).reshape(29)
    t = _real44(T).copy()
    rc = _lib.xs_host_register_step(s.ctypes.data_as(_f64p), float(damping), t.ctypes.data_as(_f64p))
    return rc == 0, t


def transform_candidates_free(n, centroid_this, centroid_other, box_t):
    """n transforms [n, 4, 4] float64 that cover SO(3) with no guess (xs_host_align_search_free, CPU): candidate i's rotation is Shoemake's
    uniform-quaternion map at the Halton point (i + 1; bases 2, 3, 5), its translation takes this map's centroid onto the other's, plus
    box_t (2 halton(i + 1; 7, 11, 13) - 1) metres.  ValueError: n < 1, an input that is not finite, a negative box."""
    a, b = (np.ascontiguousarray(c, np.float64).reshape(3) for c in (centroid_this, centroid_other))
    out = np.zeros((max(int(n), 0), 4, 4), np.float64)
    if _lib.xs_host_align_search_free(int(n), a.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p), float(box_t), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("transform_candidates_free: n < 1, an input that is not finite or a negative box")
    return out


def transform_candidates_around(T, pivot, box_t, box_r, n):
    """n transforms [n, 4, 4] float64 about T (xs_host_align_search_around, CPU): entry 0 is T itself; entry i >= 1 turns T by
    exp(box_r u[3:6]) about the image of `pivot` under T and shifts it by box_t u[0:3], u = 2 halton(i; 2, 3, 5, 7, 11, 13) - 1.
    ValueError: n < 1, an input that is not finite, a negative box."""
    t, p = _real44(T), np.ascontiguousarray(pivot, np.float64).reshape(3)
    out = np.zeros((max(int(n), 0), 4, 4), np.float64)
    if _lib.xs_host_align_search_around(t.ctypes.data_as(_f64p), p.ctypes.data_as(_f64p), float(box_t), float(box_r), int(n), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("transform_candidates_around: n < 1, an input that is not finite or a negative box")
    return out


def transform_rank(out2xP, keep):
    """The min(keep, P) indices of out2xP [P, 2] ({sum r^2, count}) with the highest S = count - sum r^2, best first, ties to the lower
    index (xs_host_align_search_rank, CPU)."""
    o = np.ascontiguousarray(out2xP, np.float64).reshape(-1, 2)
    idx = np.zeros(max(min(int(keep), o.shape[0]), 1), np.int32)
    n = _lib.xs_host_align_search_rank(o.ctypes.data_as(_f64p), o.shape[0], int(keep), idx.ctypes.data_as(_i32p))
    return idx[:n].copy()


def band_centroid(keys, voxel_size):
    """The centroid [3] (metres) of the voxel centres of packed band keys (x | y << 21 | z << 42): exact integer sums, then (sum / count + 0.5)
    voxel_size (xs_host_band_centroid, CPU).  ValueError for no key."""
    k = np.ascontiguousarray(keys).view(np.uint64).reshape(-1)
    out = np.zeros(3, np.float64)
    if _lib.xs_host_band_centroid(k.ctypes.data_as(C.POINTER(C.c_uint64)), k.size, float(voxel_size), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("band_centroid: no key")
    return out


def points_centroid(points, stride=1):
    """The centroid [3] float64 of every stride-th point of a host cloud [N, 3] float32: each axis added in double in index order, divided by
    the count (xs_host_points_centroid, CPU): the cloud centroid register_points_global matches to the map's.  ValueError for no point or
    stride < 1."""
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(3, np.float64)
    if _lib.xs_host_points_centroid(p.ctypes.data_as(_f32p), p.shape[0], int(stride), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("points_centroid: no point, or stride < 1")
    return out


def merge_tile_box(xform12, lo, hi, src_res):
    """The merge kernel's cull box (CPU): (lo [3], hi [3]) inclusive source voxel indices that contain every source voxel a destination voxel
    of the tile lo .. hi (inclusive) reads, or None when no voxel of the tile falls inside the source."""
    m = np.ascontiguousarray(xform12, np.float32).reshape(12)
    l, h, s = (np.ascontiguousarray(a, np.int32).reshape(3) for a in (lo, hi, src_res))
    box = np.zeros(6, np.int32)
    rc = _lib.xs_host_merge_tile_box(m.ctypes.data_as(_f32p), l.ctypes.data_as(_i32p), h.ctypes.data_as(_i32p), s.ctypes.data_as(_i32p), box.ctypes.data_as(_i32p))
    return (box[:3].copy(), box[3:].copy()) if rc == 1 else None


CHECKPOINT_ERRORS = ("ok", "magic", "geometry", "brick_edge", "reserved", "brick_grid", "poses", "class_byte", "payload_words", "length")


def checkpoint_info(path):
    """What a checkpoint file of either format holds (CPU; no payload is read): a dict with version (2: dense XSTSDF2, 3: brick-sparse XSTSDF3),
    valid (the format's full validation: header fields, every class byte, the sum of the words per class, the exact file length), error (one of
    CHECKPOINT_ERRORS), res, voxel_size, tranc_dist, frame_id, n_poses, planes (zs0, zs1), shard (rank, count), file_bytes, payload_words and,
    for version 3, brick_edge, brick_grid, bricks and classes (bricks per class 0 .. 7).  ValueError for a file that is neither."""
    o = np.zeros(32, np.float64)
    if _lib.xs_host_checkpoint_info(str(path).encode(), o.ctypes.data_as(_f64p)) != 0:
        raise ValueError(f"checkpoint_info: {path} is not a checkpoint file")
    i = lambda k: int(o[k])
    info = dict(version=i(0), valid=bool(o[1]), error=CHECKPOINT_ERRORS[i(28)], res=(i(2), i(3), i(4)), voxel_size=float(np.float32(o[5])),
                tranc_dist=float(np.float32(o[6])), frame_id=i(7), n_poses=i(8), planes=(i(9), i(10)), shard=(i(11), i(12)), file_bytes=i(27),
                payload_words=i(26))
    if info["version"] == 3:
        info.update(brick_edge=i(13), brick_grid=(i(14), i(15), i(16)), bricks=i(17), classes=[i(18 + c) for c in range(8)])
    return info


def _halton(i, base):
    """The radical inverse of the integer i >= 1 in `base` (float64)."""
    f, r = 1.0, 0.0
    while i > 0:
        f /= base
        r += f * (i % base)
        i //= base
    return r


def _se3_exp(xi):
    """The exponential of the real twist (v, omega) as a 4 x 4 matrix, float64."""
    v, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-12:
        R, V = np.eye(3) + K, np.eye(3) + K
    else:
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, V @ v
    return T


POSE_CANDIDATE_PRIMES = (2, 3, 5, 7, 11, 13)


def pose_candidates(center_c2v, box_t, box_r, n):
    """n camera2volume hypotheses [n, 4, 4, 2] float32 (zero imaginary parts) around center_c2v ([4, 4, 2] or real [4, 4]) for
    KinectFusion.relocalize_global: candidate i = center @ se3Exp(twist_i), a camera-frame move by the twist
    (u[:3] * box_t metres, u[3:] * box_r radians) with u_j = 2 halton(i + 1, prime_j) - 1 in (-1, 1), primes 2, 3, 5, 7, 11, 13 — a
    low-discrepancy cover of the box, the same for every call (CPU, numpy)."""
    c = np.asarray(center_c2v, np.float64)
    c = c[..., 0] if c.ndim == 3 else c
    assert c.shape == (4, 4)
    out = np.zeros((int(n), 4, 4, 2), np.float32)
    for i in range(int(n)):
        u = np.array([2.0 * _halton(i + 1, b) - 1.0 for b in POSE_CANDIDATE_PRIMES])
        out[i, ..., 0] = c @ _se3_exp(np.concatenate([u[:3] * float(box_t), u[3:] * float(box_r)]))
    return out


def flat_yaml_get(text, key):
    buf = C.create_string_buffer(1024)
    n = _lib.xs_flat_yaml_get(text.encode(), key.encode(), buf, 1024)
    return None if n < 0 else buf.value.decode()


def set_stream(stream):
    _lib.xs_kf_set_stream(None if stream is None else (stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)))


class Mesh(collections.namedtuple("Mesh", "vertices vertex_im normals triangles edge_keys")):
    """A triangle mesh of the TSDF (KinectFusion.export_mesh): numpy arrays, vertices in ascending edge key."""


class MapDiff(collections.namedtuple("MapDiff", "counts only_this only_other masks")):
    """What differs between two maps (KinectFusion.diff_map): counts, a dict of compared, only_this and only_other voxels; only_this and
    only_other, the clusters of each class as structured arrays of KinectFusion.FRONTIER_DTYPE; masks, the pair (only_this, only_other) of
    uint8 [Z, Y, X] or None."""


class RenderedViews(collections.namedtuple("RenderedViews", "depth depth_u16 normal shade counts")):
    """What KinectFusion.render_views returns for P views of rows x cols pixels: depth float32 [P, rows, cols] (metres along the camera's z, 0 without
    a hit), depth_u16 uint16 [P, rows, cols] (millimetres, what process_frame and relocalize take), normal float32 [P, 3, rows, cols] (volume
    frame, pointing into free space, NaN without one), shade uint8 [P, rows, cols] (headlight shading, 0 without a normal) and counts uint32
    [P, 4] = {hit, backface, rejected, none} rays.  An output that was not asked for is None."""


class MapSamples(collections.namedtuple("MapSamples", "status value dvalue gradient counts")):
    """What KinectFusion.sample returns for N points: status uint8 [N] (capi.SAMPLE_OUTSIDE 0, SAMPLE_UNSEEN 1, SAMPLE_OK 2), value float32 [N] (the
    trilinear TSDF in units of the truncation distance, NaN where the status is not OK), dvalue float32 [N] (the grad volume interpolated the
    same way), gradient float32 [N, 3] (value per metre, NaN where one of its six samples is refused) and counts uint64 [4] = {outside, unseen, ok,
    no_depth} (int64 as a torch tensor).  An output that was not asked for is None."""


class FrameResiduals(collections.namedtuple("FrameResiduals", "status value dvalue gradient counts")):
    """What KinectFusion.frame_residuals returns: MapSamples' fields as images, status and the floats [rows, cols], gradient [3, rows, cols]; a pixel
    without a usable depth has status capi.SAMPLE_NO_DEPTH (3)."""


def sample_compose(T_a2v, T_p2a):
    """T = T_a2v T_p2a (real 4 x 4, float64) for KinectFusion.sample: the points are in a frame P whose pose in frame A is T_p2a, and T_a2v takes A to
    the volume (CPU)."""
    a, b, out = _real44(T_a2v), _real44(T_p2a), np.zeros(16, np.float64)
    if _lib.xs_host_sample_compose(a.ctypes.data_as(_f64p), b.ctypes.data_as(_f64p), out.ctypes.data_as(_f64p)) != 0:
        raise ValueError("sample_compose: two 4 x 4 matrices are needed")
    return out.reshape(4, 4)


def save_view_pgm(path, shade):
    """One rendered image (uint8 [rows, cols], e.g. RenderedViews.shade[p]) as a binary P5 file."""
    a = shade.cpu().numpy() if hasattr(shade, "cpu") else np.asarray(shade)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("save_view_pgm: a uint8 image [rows, cols] is needed")
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (a.shape[1], a.shape[0]))
        f.write(np.ascontiguousarray(a).tobytes())
