"""What the instance methods share around a C call, each step once: argument arrays (returned as arrays, which the caller holds until the
call has returned), output buffers, search options, report vectors, the return-code check and the capacity retry."""
import numpy as np

from . import capi
from .pipeline_abi import _f64p, _vp


def pose_stack(c2vs):
    """(flat float32 array, P) of camera2volume poses [P, 4, 4, 2]."""
    m = np.ascontiguousarray(c2vs, dtype=np.float32).reshape(-1)
    P = m.size // 32
    assert m.size == 32 * P
    return m, P


def points_arg(name, points):
    """(n, address, on_device, the array to keep alive) of a cloud: a numpy array [N, 3] or a contiguous float32 torch tensor on the GPU."""
    if hasattr(points, "data_ptr"):   # a torch tensor on the GPU
        if not points.is_cuda or not points.is_contiguous() or points.dim() != 2 or points.shape[1] != 3 or points.element_size() != 4 or not points.is_floating_point():
            raise ValueError(f"{name}: a torch points tensor must be contiguous float32 [N, 3] on the GPU")
        n, pp, on_device, keep = int(points.shape[0]), points.data_ptr(), 1, points
    else:
        keep = np.ascontiguousarray(points, dtype=np.float32)
        if keep.ndim != 2 or keep.shape[1] != 3:
            raise ValueError(f"{name}: points must be [N, 3]")
        n, pp, on_device = keep.shape[0], keep.ctypes.data, 0
    if n < 1:
        raise ValueError(f"{name}: at least one point is needed")
    return n, pp, on_device, keep


def transform_stack(Ts):
    """Real transforms, one [4, 4] or a stack, as float64 [N, 4, 4]."""
    return np.ascontiguousarray(np.asarray(Ts, dtype=np.float64).reshape(-1, 4, 4))


def optional(a, size):
    """A float32 vector of `size` entries (a pose [4, 4, 2], intrinsics), or None."""
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(size)


def ptr(a, pointer_type):
    """The argument for an array the caller holds; a null pointer for None."""
    return None if a is None else a.ctypes.data_as(pointer_type)


def depth_pointers(depths):
    """The C array of the addresses of a list of device depth images (torch tensors or raw addresses)."""
    return (_vp * max(len(depths), 1))(*[d if isinstance(d, int) else d.data_ptr() for d in depths])


def output_buffers(name, outputs, shapes, device):
    """(dict of numpy arrays, or with device of torch tensors on the GPU, dict of their addresses) for the outputs asked for, of
    shapes = {output: (shape, numpy dtype)}.  Where torch lacks an unsigned type the signed one of the same width carries the bits."""
    wanted = set(outputs)
    if not wanted or not wanted <= set(shapes):
        raise ValueError(f"{name}: outputs must name some of {', '.join(shapes)}")
    out, ptrs = {}, {}
    if device:
        import torch
        dt = {np.float32: torch.float32, np.uint8: torch.uint8, np.uint16: getattr(torch, "uint16", torch.int16), np.uint32: torch.int32, np.uint64: torch.int64}
    for n in wanted:
        shape, dtype = shapes[n]
        if device:
            out[n] = torch.empty(shape, dtype=dt[dtype], device="cuda")
            ptrs[n] = out[n].data_ptr()
        else:
            out[n] = np.zeros(shape, dtype)
            ptrs[n] = out[n].ctypes.data
    return out, ptrs


def fill_search_opts(o, candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations, damping, min_weight, max_residual, Ts):
    """Fills a search-options struct that holds the library's defaults (box_t, refine_t None keep theirs); returns the array it points into."""
    o.candidates, o.keep, o.rounds, o.stride, o.iterations, o.min_weight = int(candidates), int(keep), int(rounds), int(stride), int(iterations), int(min_weight)
    if box_t is not None:
        o.box_t = float(box_t)
    if refine_t is not None:
        o.refine_t = float(refine_t)
    o.refine_r, o.damping, o.max_residual = float(refine_r), float(damping), float(max_residual)
    if Ts is None:
        return None
    user = transform_stack(Ts)
    o.user_n, o.user_T16xN = user.shape[0], user.ctypes.data_as(_f64p)
    return user


# the report vectors of the C calls, entry by entry
_GN_REPORT = (("start", int), ("count", int), ("sum_r2", float), ("loss", float), ("passes", int), ("ended_ok", int))
ALIGN_REPORT = _GN_REPORT + (("band_voxels", int),)
REGISTER_REPORT = _GN_REPORT + (("points", int),)
_SEARCH_REPORT = (("rank", int), ("S_before", float), ("count", int), ("sum_r2", float), ("loss", float), ("score_launches", int), ("passes", int), ("ended_ok", int))
ALIGN_SEARCH_REPORT = _SEARCH_REPORT + (("band_voxels", int), ("scored_entries", int), ("centroid_distance", float))
REGISTER_SEARCH_REPORT = _SEARCH_REPORT + (("points", int), ("scored_points", int), ("centroid_distance", float))
RELOCALIZE_REPORT = (("index", int), ("S_before", float), ("S_after", float), ("sum_loss_after", float), ("count_after", float), ("refined_ok", int), ("index_voxels", int))


def report(vector, keys):
    """A report vector as a dict, from its (key, type) per entry."""
    return {k: t(vector[i]) for i, (k, t) in enumerate(keys)}


def check_rc(name, rc, shard="", bad=-1, bad_text="bad arguments or options", zero_ok=False, rest=None, rest_ok=False):
    """What a call's return code raises; returns rc when it is a result (1: success).  -2: XsError, shard mode, for the reason `shard`
    (None: the call has no such code).  `bad`, the call's code for bad arguments (-1; -3 where -1 is an index): ValueError with bad_text.
    0: "no volume", or a result with zero_ok.  Any other code: a result with rest_ok, else ValueError with `rest` (None: the code)."""
    if rc == -2 and shard is not None:
        raise capi.XsError(f"{name}: not available in shard mode" + (f" ({shard})" if shard else ""))
    if rc == bad:
        raise ValueError(f"{name}: {bad_text}")
    if rc == 1 or rest_ok or (zero_ok and rc == 0):
        return rc
    raise ValueError(f"{name}: no volume" if rc == 0 else f"{name}: {rc if rest is None else rest}")


def retry_capacity(run, capacity):
    """run(capacity) -> (return code, the count the call reported, its buffers); on -4, too little room, once more with that count."""
    for _ in range(2):
        rc, needed, buffers = run(capacity)
        if rc != -4:
            break
        capacity = needed
    return rc, buffers
