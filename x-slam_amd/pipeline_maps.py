"""KinectFusion's operations on whole maps, off the frame path: merge, difference, alignment, rendering, sampling, point-cloud registration
and fusion, taking fused frames out again.  pipeline_abi._MAP_SOURCES says which C entry point takes the map from where."""
import ctypes as C

import numpy as np

from . import capi
from .pipeline_abi import _MAP_SOURCES, AlignSearchOpts, RegisterSearchOpts, _f32p, _f64p, _i32p, _lib
from .pipeline_hostmath import FrameResiduals, MapDiff, MapSamples, RenderedViews, _real44
from .pipeline_marshal import (ALIGN_REPORT, ALIGN_SEARCH_REPORT, REGISTER_REPORT, REGISTER_SEARCH_REPORT, check_rc, depth_pointers, fill_search_opts, optional,
                               output_buffers, points_arg, ptr, report, retry_capacity, transform_stack)

_BAD_SEARCH = "T not finite, a count, stride, box, min_weight, max_residual or damping out of range"
_RENDER_DEFAULTS = dict(intr=None, size=None, t_near=0.2, t_far=5.0, step=None, min_weight=1, outputs=("depth", "normal", "shade"), cull=True, device=False)


def _map_rc(name, rc, bad, zero_ok=False):
    """check_rc for a call that reads a map; `bad` names the call's own bad arguments, zero_ok: 0 is "no result", not "no volume"."""
    check_rc(name, rc, bad_text=f"bad arguments ({bad}, the volume itself as source, a bad file or another truncation distance)", zero_ok=zero_ok)


class Maps:
    """Mixin of KinectFusion (pipeline.py), which provides h, cfg, res, width and height; _cluster_records is Planning's."""

    def _source(self, family, other=None, path=None):
        """(C name, ctypes function, leading arguments) of a family's call on this instance's map, on `other`'s or on the checkpoint at `path`."""
        own, instance, checkpoint = _MAP_SOURCES[family][0]
        name, lead = own, (self.h,)
        if other is not None:
            name, lead = instance, (self.h, other.h)
        elif path is not None:
            name, lead = checkpoint, (self.h, path.encode())
        return name, getattr(_lib, name), lead

    def _merge_call(self, source, T, min_weight):
        name, fn, lead = source
        t = _real44(np.eye(4) if T is None else T)
        n = C.c_ulonglong(0)
        _map_rc(name, fn(*lead, t.ctypes.data_as(_f64p), int(min_weight), C.byref(n)), "T not finite, min_weight < 1")
        return int(n.value)

    def merge_map(self, other, T=None, min_weight=1):
        """Merges the map of `other` (another KinectFusion of this process; only read) into this one: its volume is resampled into this map's
        voxel grid under T (real 4 x 4: a point of THIS map's volume frame, in metres, to the other map's; None: the identity) and averaged in by
        weight as a new observation is, where all the corners it is interpolated from carry min_weight.  Resolutions and voxel sizes may
        differ, the truncation distances may not.  Everything derived from the volume follows; poses and the frame number do not change.
        Returns the number of voxels written.  XsError in shard mode, ValueError on bad arguments (the state is unchanged)."""
        return self._merge_call(self._source("merge", other=other), T, min_weight)

    def merge_checkpoint(self, path, T=None, min_weight=1):
        """merge_map with the other map read from a checkpoint file of a whole volume (save_checkpoint, dense or sparse: either format is accepted); the file is validated before anything
        is touched and a bad one raises ValueError with the state unchanged."""
        return self._merge_call(self._source("merge", path=path), T, min_weight)

    def _reintegrate_call(self, depths, c2v_olds, c2v_news, modes, frames):
        n = len(depths)
        if n < 1 or len(modes) != n:
            raise ValueError("reintegrate: at least one frame, one mode per frame")
        P = depth_pointers(depths)

        def poses(c):
            a = optional(c, -1)
            if a is not None and a.size != 32 * n:
                raise ValueError("reintegrate: one camera2volume [4, 4, 2] per frame")
            return a

        olds, news = poses(c2v_olds), poses(c2v_news)
        mode = np.ascontiguousarray(modes, np.int32)
        idx = None if frames is None else np.ascontiguousarray([-1 if f is None else int(f) for f in frames], np.int32)
        if idx is not None and idx.size != n:
            raise ValueError("reintegrate: one frame index (or None) per frame")
        counts = (C.c_ulonglong * 4)()
        rc = _lib.xs_kf_reintegrate(self.h, n, P, self.width * 2, ptr(olds, _f32p), ptr(news, _f32p), mode.ctypes.data_as(_i32p), ptr(idx, _i32p), counts)
        bad = "bad arguments (a pose that is not finite, a frame index past the record)"
        check_rc("reintegrate", rc, bad_text=bad, rest=bad)
        return dict(removed=int(counts[0]), added=int(counts[1]), emptied=int(counts[2]), orphaned=int(counts[3]))

    def deintegrate(self, depth_dev, c2v):
        """Takes the depth frame (torch CUDA tensor [H, W], u16 millimetres) fused at camera2volume c2v [4, 4, 2] out of the volume again: every
        voxel the frame wrote loses that observation from its running mean and one unit of weight; a voxel it alone had written is empty
        again.  Exact up to rounding while no weight had reached max_integration_weight (include/xslam_amd.h: what removal cannot undo).
        Everything derived from the volume follows, as after merge_map; poses and the frame number do not change.  Returns the counts
        dict(removed, added, emptied, orphaned) in voxels; orphaned: the frame would have written there but nothing was left to take.
        XsError in shard mode, ValueError on bad arguments (the state is unchanged)."""
        return self._reintegrate_call([depth_dev], [c2v], None, [1], None)

    def reintegrate(self, depth_dev, c2v_old, c2v_new, frame=None):
        """deintegrate at c2v_old and fuse the same frame again at c2v_new, in one pass over the volume.  frame: the index of that frame in the
        pose record (world2camera(frame)), which then receives the pose that gives c2v_new.  Returns the counts."""
        return self._reintegrate_call([depth_dev], [c2v_old], [c2v_new], [3], None if frame is None else [frame])

    def reintegrate_batch(self, depths, c2v_olds, c2v_news, frames=None):
        """reintegrate for several frames: the observations are applied in list order, up to eight per pass over the volume, and the derived
        state is rebuilt once.  The volume equals the one the single calls in the same order leave, bit for bit.  Returns the summed counts."""
        return self._reintegrate_call(list(depths), c2v_olds, c2v_news, [3] * len(depths), frames)

    def refine_frame(self, depth_dev, c2v, iterations=5, damping=1e-3, frame=None):
        """Refines the pose of a frame that is already fused: takes it out at c2v, runs relocalize against the map without it starting at c2v —
        a map that still holds the frame pulls the refinement towards where the frame already is — and puts it back at the refined pose, or at
        c2v again if the refinement failed.  Returns (ok, refined c2v [4, 4, 2], loss history, counts of both edits summed)."""
        c2v = np.ascontiguousarray(c2v, dtype=np.float32).reshape(4, 4, 2)
        out = self.deintegrate(depth_dev, c2v)
        ok, refined, hist = self.relocalize(depth_dev, c2v, iterations=iterations, damping=damping)
        ok = bool(ok) and bool(np.isfinite(refined).all())
        back = self._reintegrate_call([depth_dev], None, [refined if ok else c2v], [2], None if frame is None or not ok else [frame])
        return ok, (refined if ok else c2v), hist, {k: out[k] + back[k] for k in out}

    def _render_call(self, source, c2vs, intr, size, t_near, t_far, step, min_weight, outputs, cull, device):
        name, fn, lead = source
        m = np.ascontiguousarray(c2vs, dtype=np.float32)
        if m.ndim == 2 or (m.ndim == 3 and m.shape[-1] == 2):
            m = m[None]
        if m.shape[1:] not in ((4, 4), (4, 4, 2)) or m.shape[0] < 1:
            raise ValueError(f"{name}: c2vs must be [P, 4, 4] or [P, 4, 4, 2]")
        P, is_complex = m.shape[0], int(m.ndim == 4)
        m = m.reshape(-1)
        k = optional(intr, 4)
        rows, cols = (self.height, self.width) if size is None else (int(size[0]), int(size[1]))
        out, at = output_buffers(name, outputs, dict(depth=((P, rows, cols), np.float32), depth_u16=((P, rows, cols), np.uint16), normal=((P, 3, rows, cols), np.float32),
                                                     shade=((P, rows, cols), np.uint8), counts=((P, 4), np.uint32)), device)
        opts = capi.render_opts(t_near, t_far, step, min_weight, cull)
        rc = fn(*lead, P, m.ctypes.data_as(_f32p), is_complex, ptr(k, _f32p), rows, cols, C.byref(opts), *(at.get(n) for n in RenderedViews._fields), int(bool(device)))
        _map_rc(name, rc, "poses, intrinsics or size out of range or not finite, t_far <= t_near, more than 4096 samples, a map that cannot be rendered")
        return RenderedViews(*(out.get(n) for n in RenderedViews._fields))

    def render_views(self, c2vs, intr=None, size=None, t_near=0.2, t_far=5.0, step=None, min_weight=1, outputs=("depth", "normal", "shade"), cull=True,
                     device=False):
        """Views of the map from P poses the caller picks, c2vs [P, 4, 4] or [P, 4, 4, 2] camera-to-volume (real parts; camera2volume() gives one),
        64 views per launch: a RenderedViews of the `outputs` asked for (depth, depth_u16, normal, shade, counts), numpy arrays, or torch tensors
        on the GPU with device=True.  intr (fx, fy, cx, cy) and size (rows, cols) default to the configuration's camera; depths t_near .. t_far
        along the camera's z in increments of `step` (None: a voxel); a voxel with a weight below min_weight is unseen.  cull=False reads every
        sample instead of consulting the brick mask: the same bits, slower.  depth_u16 is what a depth sensor at that pose would deliver, so it
        can stand in for a frame: relocalize(views.depth_u16[p], c2v) with device=True.  counts says how the rays ended; a crossing whose two
        trilinear values do not bracket zero is rejected, which a step of two or three voxels makes rarer than a step of one (DESIGN.md section
        4.28).  XsError in shard mode, ValueError on bad arguments."""
        return self._render_call(self._source("render"), c2vs, intr, size, t_near, t_far, step, min_weight, outputs, cull, device)

    def render_map(self, other, c2vs, **kw):
        """render_views of the map of `other` (another KinectFusion of this process, which is only read); the poses are in ITS volume frame, the
        default camera is this instance's."""
        return self._render_call(self._source("render", other=other), c2vs, **{**_RENDER_DEFAULTS, **kw})

    def render_checkpoint(self, path, c2vs, **kw):
        """render_views of the map in a checkpoint file of a whole volume (save_checkpoint, dense or sparse), validated as merge_checkpoint does."""
        return self._render_call(self._source("render", path=path), c2vs, **{**_RENDER_DEFAULTS, **kw})

    def _sample_call(self, source, points, T, min_weight, outputs, device):
        name, fn, lead = source
        n, pp, on_device, keep = points_arg(name, points)
        t = None if T is None else _real44(T)
        out, at = output_buffers(name, outputs, dict(status=((n,), np.uint8), value=((n,), np.float32), dvalue=((n,), np.float32), gradient=((n, 3), np.float32),
                                                     counts=((4,), np.uint64)), device)
        rc = fn(*lead, n, pp, ptr(t, _f64p), int(min_weight), *(at.get(f) for f in MapSamples._fields), on_device | (2 if device else 0))
        _map_rc(name, rc, "more than 2^30 points, T not finite, dvalue of a map without a grad array")
        return MapSamples(*(out.get(f) for f in MapSamples._fields))

    def sample(self, points, T=None, min_weight=1, outputs=("status", "value", "gradient"), device=False):
        """The map asked at N points: what is the signed distance here, which way does it grow, has this place been seen.  points [N, 3] in metres,
        a numpy array or a contiguous float32 torch tensor on the GPU, in a frame that T (real 4 x 4; None: they are in the volume frame already
        and their bits are used as they are) takes to the volume frame.  Returns a MapSamples of the `outputs` asked for (status, value, dvalue,
        gradient, counts): numpy arrays, or torch tensors on the GPU with device=True.  value is the trilinear interpolation of the stored TSDF
        (the render's F, bit for bit), which is normalised by the truncation distance: value * tranc_dist() is the signed distance in metres
        near the surface, positive in free space, and the field is TRUNCATED: farther than tranc_dist() from the surface it is +-1 and says
        only which side the point is on, or the point is UNSEEN.  gradient is the central difference over one voxel, in value per metre: it
        points into free space with a length of about 1 / tranc_dist() near the surface.  dvalue is the same interpolation of the run's
        derivative volume (the CSFD seed's).  A voxel with a weight below min_weight is unseen.  XsError in shard mode, ValueError on bad
        arguments."""
        return self._sample_call(self._source("sample"), points, T, min_weight, outputs, device)

    def sample_map(self, other, points, T=None, min_weight=1, outputs=("status", "value", "gradient"), device=False):
        """sample of the map of `other` (another KinectFusion of this process, which is only read); T takes the points to ITS volume frame."""
        return self._sample_call(self._source("sample", other=other), points, T, min_weight, outputs, device)

    def sample_checkpoint(self, path, points, T=None, min_weight=1, outputs=("status", "value", "gradient"), device=False):
        """sample of the map in a checkpoint file of a whole volume (save_checkpoint, dense or sparse), validated as merge_checkpoint does."""
        return self._sample_call(self._source("sample", path=path), points, T, min_weight, outputs, device)

    def frame_residuals(self, depth, c2v, min_weight=1, outputs=("status", "value"), device=False, intr=None):
        """A depth frame judged against the map before it is fused: every pixel's point (depth [rows, cols] u16 millimetres, a numpy array or a torch
        tensor on the GPU; unprojected with intr, None: the configuration's, and placed by the camera2volume c2v [4, 4] or [4, 4, 2]) sampled in
        the map.  Returns a FrameResiduals of images: value is the pixel's signed residual in units of the truncation distance (0 on the
        surface the map holds; large where an object moved or the pose is off), status says why a pixel has none."""
        m = np.ascontiguousarray(c2v, dtype=np.float32)
        if m.shape not in ((4, 4), (4, 4, 2)):
            raise ValueError("frame_residuals: c2v must be [4, 4] or [4, 4, 2]")
        if hasattr(depth, "data_ptr"):
            if not depth.is_cuda or depth.dim() != 2 or depth.element_size() != 2 or depth.stride(1) != 1:
                raise ValueError("frame_residuals: a torch depth image must be 16-bit [rows, cols] on the GPU")
            rows, cols, dp, step, on_device, keep = int(depth.shape[0]), int(depth.shape[1]), depth.data_ptr(), depth.stride(0) * 2, 1, depth
        else:
            keep = np.ascontiguousarray(depth, dtype=np.uint16)
            if keep.ndim != 2:
                raise ValueError("frame_residuals: depth must be [rows, cols]")
            rows, cols, dp, step, on_device = keep.shape[0], keep.shape[1], keep.ctypes.data, keep.shape[1] * 2, 0
        k = optional(intr, 4)
        name = "xs_kf_frame_residuals"
        shape = (rows, cols)
        out, at = output_buffers(name, outputs, dict(status=(shape, np.uint8), value=(shape, np.float32), dvalue=(shape, np.float32),
                                                     gradient=((3,) + shape, np.float32), counts=((4,), np.uint64)), device)
        rc = _lib.xs_kf_frame_residuals(self.h, dp, step, m.reshape(-1).ctypes.data_as(_f32p), int(m.ndim == 3), ptr(k, _f32p), rows, cols,
                                        int(min_weight), *(at.get(f) for f in FrameResiduals._fields), on_device | (2 if device else 0))
        _map_rc(name, rc, "an empty or oversized image, a pose or intrinsics that are not finite")
        return FrameResiduals(*(out.get(f) for f in FrameResiduals._fields))

    def surface_error(self, points, T=None, min_weight=1):
        """How far a set of surface points (a ground-truth scan, another sensor's cloud) lies from the surface the map holds: a dict of the counts
        outside, unseen and ok, and over the OK points mean_abs, rms and max_abs of d = value * tranc_dist() in metres (NaN without an OK point).
        Float64 host arithmetic on sample's value output.  The field is truncated: a point farther than tranc_dist() from the surface
        contributes tranc_dist()."""
        s = self.sample(points, T=T, min_weight=min_weight, outputs=("status", "value", "counts"))
        d = s.value[s.status == capi.SAMPLE_OK].astype(np.float64) * float(self.tranc_dist())
        stats = dict(mean_abs=float(np.abs(d).mean()), rms=float(np.sqrt((d * d).mean())), max_abs=float(np.abs(d).max())) if d.size else \
            dict(mean_abs=float("nan"), rms=float("nan"), max_abs=float("nan"))
        return dict(outside=int(s.counts[0]), unseen=int(s.counts[1]), ok=int(s.counts[2]), **stats)

    def _diff_call(self, source, T, min_weight, lo, hi, cell_vox, min_size, masks, capacity):
        name, fn, lead = source
        t = _real44(np.eye(4) if T is None else T)
        u64p = C.POINTER(C.c_uint64)
        dense = [np.zeros((self.res[2], self.res[1], self.res[0]), np.uint8) for _ in range(2)] if masks else None
        dp = [d.ctypes.data_as(C.POINTER(C.c_ubyte)) for d in dense] if masks else [None, None]
        counts, n_this, n_other = np.zeros(3, np.uint64), C.c_int(0), C.c_int(0)

        def run(capacity):
            recs = [np.zeros((max(capacity, 1), capi.FRONTIER_RECORD_WORDS), np.uint64) for _ in range(2)]
            rc = fn(*lead, t.ctypes.data_as(_f64p), int(min_weight), float(lo), float(hi), int(cell_vox), int(min_size), capacity,
                    recs[0].ctypes.data_as(u64p), C.byref(n_this), recs[1].ctypes.data_as(u64p), C.byref(n_other),
                    counts.ctypes.data_as(C.POINTER(C.c_ulonglong)), dp[0], dp[1])
            return rc, max(int(n_this.value), int(n_other.value)), recs

        rc, recs = retry_capacity(run, capacity)
        _map_rc(name, rc, "T, lo or hi not finite, lo > hi, min_weight < 1, a bad cell")
        return MapDiff(dict(compared=int(counts[0]), only_this=int(counts[1]), only_other=int(counts[2])), self._cluster_records(recs[0][:n_this.value]),
                       self._cluster_records(recs[1][:n_other.value]), tuple(dense) if masks else None)

    def diff_map(self, other, T=None, min_weight=1, lo=0.0, hi=0.5, cell_vox=0, min_size=8, masks=False, capacity=1024):
        """What differs between this map and the map of `other` (another KinectFusion of this process), with nothing averaged: THIS map is
        self, the OTHER map is `other` resampled into this map's voxel grid under T as merge_map does it (real 4 x 4: a point of this map's
        volume frame, in metres, to the other map's; None: the identity).  A voxel is compared where both maps carry min_weight; it is
        only_this where this map's value is below lo and the other's at least hi (matter here, firmly free there) and only_other the other
        way round.  With `other` the earlier map, only_this is what appeared and only_other what went away.  Returns a MapDiff: counts (a
        dict of compared, only_this and only_other voxels), only_this and only_other (the clusters of each class with at least min_size voxels,
        26-adjacency within cells of cell_vox voxels, 0: the whole volume, as frontiers() returns them) and masks (the pair of uint8 [Z, Y, X],
        with masks=True).  capacity: the first guess at the number of clusters per class; a longer list is fetched by a second run.  Nothing
        of either map is modified.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.diff_map(other, kf.align_map_global(other)[1])."""
        return self._diff_call(self._source("diff", other=other), T, min_weight, lo, hi, cell_vox, min_size, masks, int(capacity))

    def diff_checkpoint(self, path, T=None, min_weight=1, lo=0.0, hi=0.5, cell_vox=0, min_size=8, masks=False, capacity=1024):
        """diff_map with the other map read from a checkpoint file of a whole volume (save_checkpoint, dense or sparse: either format is accepted), validated as merge_checkpoint does: with
        yesterday's checkpoint as the other map, only_this is what appeared since and only_other what went away.
        Intended use: kf.diff_checkpoint(path, kf.align_checkpoint_global(path)[1])."""
        return self._diff_call(self._source("diff", path=path), T, min_weight, lo, hi, cell_vox, min_size, masks, int(capacity))

    def _align_call(self, source, T0, iterations, damping, min_weight, max_residual, cloud=(), keys=ALIGN_REPORT, bad=""):
        """(ok, T, report, loss history) of the Gauss-Newton loop of the align calls and, with `cloud` (points_arg's result), the register calls."""
        name, fn, lead = source
        t = transform_stack(np.eye(4) if T0 is None else T0)
        iterations = int(iterations)
        out, rep, hist = np.zeros((4, 4), np.float64), np.zeros(8, np.float64), np.zeros(max(iterations, 0) + 1, np.float64)
        rc = fn(*lead, *cloud[:3], t.ctypes.data_as(_f64p), t.shape[0], iterations, float(damping), int(min_weight), float(max_residual),
                out.ctypes.data_as(_f64p), rep.ctypes.data_as(_f64p), hist.ctypes.data_as(_f64p))
        _map_rc(name, rc, bad + "T not finite, iterations < 0, min_weight < 1, max_residual or damping out of range", zero_ok=True)
        return rc == 1, (out if rc == 1 else t[0].copy()), report(rep, keys), (hist.copy() if rc == 1 else hist[:0].copy())

    def align_map(self, other, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=1.0):
        """Registers the map of `other` (another KinectFusion of this process) to this one, volume to volume, before a merge: damped Gauss-Newton
        over this map's band voxels on "the other map resampled under T minus this map", at the sample positions merge_map(other, T) will use.
        T0: a starting guess as merge_map takes T (None: the identity), or a stack [N, 4, 4] of them, refined together; the best by
        S = count - sum r^2 wins.  Returns (ok, T [4, 4] float64, report dict, loss history [iterations + 1]); ok False (T = the first start) when
        no start kept six voxels on every pass and a positive definite system.  Nothing is modified.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.merge_map(other, kf.align_map(other, T_guess)[1])."""
        return self._align_call(self._source("align", other=other), T0, iterations, damping, min_weight, max_residual)

    def align_checkpoint(self, path, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=1.0):
        """align_map with the other map read from a checkpoint file of a whole volume (save_checkpoint, dense or sparse: either format is accepted), validated as merge_checkpoint does.
        Intended use: kf.merge_checkpoint(path, kf.align_checkpoint(path, T_guess)[1])."""
        return self._align_call(self._source("align", path=path), T0, iterations, damping, min_weight, max_residual)

    def _register_call(self, source, points, *loop):
        ok, T, rep, hist = self._align_call(source, *loop, points_arg(source[0], points), REGISTER_REPORT, "more than 2^30 points, ")
        return ok, T, dict(rep, loss_history=hist)

    def register_points(self, points, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=0.9):
        """Registers a point cloud (a lidar sweep, another sensor's points, a ground-truth scan, an exported cloud of an earlier session) to this
        map: damped Gauss-Newton on "the map's value at T p" over the points, whose Jacobian is the map's gradient there, one launch per pass
        for all starts.  points [N, 3] in metres, a numpy array or a contiguous float32 torch tensor on the GPU.  T0: a starting guess (real
        4 x 4: a point of the cloud's frame to the volume frame; None: the identity), or a stack [N, 4, 4] of them, refined together; the
        best by S = count - sum r^2 among the starts that kept six points on every pass wins (align_map's rule; iterations=0 ranks the starts
        without stepping).  A point takes part where the map holds a value and a gradient at T p with min_weight and |value| <= max_residual.
        The default max_residual is 0.9 rather than align_map's 1.0: a sample of exactly +-1 is the truncated field, which has gradient 0 and
        carries no information about T, so such points only dilute the loss.  Returns (ok, T [4, 4] float64, report dict: start, count,
        sum_r2, loss, passes, ended_ok, points, loss_history [iterations + 1]); ok False (T = the first start) when no start ended ok.
        Nothing is modified.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.surface_error(scan, kf.register_points(scan, T_guess)[1])."""
        return self._register_call(self._source("register"), points, T0, iterations, damping, min_weight, max_residual)

    def register_map_points(self, other, points, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=0.9):
        """register_points against the map of `other` (another KinectFusion of this process, which is only read); T takes the points to ITS volume frame."""
        return self._register_call(self._source("register", other=other), points, T0, iterations, damping, min_weight, max_residual)

    def register_checkpoint_points(self, path, points, T0=None, iterations=10, damping=1e-3, min_weight=1, max_residual=0.9):
        """register_points against the map in a checkpoint file of a whole volume (save_checkpoint, dense or sparse), validated as merge_checkpoint does."""
        return self._register_call(self._source("register", path=path), points, T0, iterations, damping, min_weight, max_residual)

    _FUSE_COUNTS = ("used", "dropped", "visits", "outside", "written")

    def fuse_points(self, points, T=None, origin=(0.0, 0.0, 0.0), min_range=0.2, max_range=5.0, carve=False, weight=1):
        """Fuses a point cloud (a lidar sweep, another sensor's points, a ground-truth scan, an earlier session's cloud) into the map.  points [N, 3]
        in metres, a numpy array or a contiguous float32 torch tensor on the GPU, and origin, the sensor's position, both in a frame that T (real
        4 x 4, as register_points returns it; None: the volume frame, the bits as they are) takes to the volume frame.  Each point's ray from the
        origin is walked in half-voxel steps through the truncation band around the point (carve=True: from the sensor on, which turns the
        unknown space the ray crosses into free space for the planning calls, at the cost of a walk as long as the ray); a voxel the sweep
        touches receives one observation of `weight`, the mean over the rays through it of the signed distance to the point ALONG THE RAY,
        averaged in as a depth frame's is.  Rays shorter than min_range or longer than max_range are dropped.  Integer atomics only: the
        result does not depend on the order of the points, and two calls on equal maps give equal bytes.  Returns a dict of used and dropped
        points, visits (voxel additions), outside (ray samples that left the volume) and written voxels.  Everything derived from the map
        follows; poses and the frame number stay.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.fuse_points(sweep, kf.register_points(sweep, T_guess)[1], origin=sensor_position)."""
        name = "xs_kf_fuse_points"
        n, pp, on_device, keep = points_arg(name, points)
        t = None if T is None else _real44(T)
        o = np.ascontiguousarray(origin, dtype=np.float32).reshape(-1)
        if o.size != 3:
            raise ValueError(f"{name}: origin must have three entries")
        counts = (C.c_ulonglong * 5)()
        rc = _lib.xs_kf_fuse_points(self.h, n, pp, on_device, ptr(t, _f64p), o.ctypes.data_as(_f32p), float(min_range),
                                    float(max_range), int(bool(carve)), int(weight), counts)
        _map_rc(name, rc, "T, origin or a range not finite, min_range <= 0, max_range < min_range or too long, weight outside 1 .. max_integration_weight")
        return {k: int(counts[i]) for i, k in enumerate(self._FUSE_COUNTS)}

    def _score_points_call(self, source, points, *scoring):
        return self._score_transforms_call(source, *scoring, points_arg(source[0], points), "more than 2^30 points, ")

    def score_point_transforms(self, points, Ts, stride=1, min_weight=1, max_residual=0.9):
        """{sum r^2, count} [P, 2] float64 of "this map's value at T p" over every stride-th point of a cloud (as register_points takes it), for
        each T of Ts [P, 4, 4] (cloud frame to volume frame), in one launch per 4096 transforms: register_points' residual without its
        gradient, so a point counts wherever the map holds a value with min_weight and |value| <= max_residual.  S = count - sum r^2 ranks the
        transforms.  Nothing is modified.  XsError in shard mode, ValueError on bad arguments."""
        return self._score_points_call(self._source("score_points"), points, Ts, stride, min_weight, max_residual)

    def score_map_point_transforms(self, other, points, Ts, stride=1, min_weight=1, max_residual=0.9):
        """score_point_transforms against the map of `other` (another KinectFusion of this process, which is only read)."""
        return self._score_points_call(self._source("score_points", other=other), points, Ts, stride, min_weight, max_residual)

    def score_checkpoint_point_transforms(self, path, points, Ts, stride=1, min_weight=1, max_residual=0.9):
        """score_point_transforms against the map in a checkpoint file of a whole volume (either format), validated as merge_checkpoint does."""
        return self._score_points_call(self._source("score_points", path=path), points, Ts, stride, min_weight, max_residual)

    def _register_global_call(self, source, points, *search):
        """search: the search arguments, candidates .. Ts, as fill_search_opts takes them."""
        name, fn, lead = source
        n, pp, on_device, alive = points_arg(name, points)
        o = RegisterSearchOpts()
        _lib.xs_kf_register_search_defaults(self.h, C.byref(o))
        user = fill_search_opts(o, *search)   # (held until the call has returned)
        out, rep = np.eye(4, dtype=np.float64), np.zeros(12, np.float64)
        rc = fn(*lead, n, pp, on_device, C.byref(o), out.ctypes.data_as(_f64p), rep.ctypes.data_as(_f64p))
        _map_rc(name, rc, "more than 2^30 points or more than 2^24 scored ones (raise the stride), " + _BAD_SEARCH, zero_ok=True)
        return rc == 1, out, report(rep, REGISTER_SEARCH_REPORT)

    def register_points_global(self, points, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10, damping=1e-3,
                               min_weight=1, max_residual=0.9, Ts=None):
        """register_points with no starting guess: a lidar sweep taken somewhere in the mapped room, yesterday's exported cloud in another frame,
        a ground-truth scan.  `candidates` transforms that cover all rotations (transform_candidates_free; translations take the centroid of
        the scored points onto the map's band centroid, jittered by box_t metres) are scored over every stride-th point
        (score_point_transforms), the `keep` best by S = count - sum r^2 are refined over `rounds` rounds of candidates about each
        (transform_candidates_around about the cloud's centroid: boxes refine_t metres and refine_r radians, halved per round), and the kept
        transforms start register_points' loop over ALL the points.  box_t, refine_t None: the map's truncation distance.  Ts [N, 4, 4]:
        candidates of the caller's that replace the free ones.  Returns (ok, T [4, 4] float64, report dict: rank, S_before, count, sum_r2,
        loss, score_launches, passes, ended_ok, points, scored_points, centroid_distance); ok False (T = the identity) when no start ended ok
        or the map has no band voxel.  The score cannot tell a scene from its image under one of its own symmetries: a symmetric scene has
        several equally good answers and any of them may be returned.  A cloud that covers only part of the map has its centroid elsewhere:
        widen box_t.  Nothing is modified.  XsError in shard mode, ValueError on bad arguments.
        Intended use: kf.fuse_points(sweep, kf.register_points_global(sweep)[1], origin=sensor_position)."""
        return self._register_global_call(self._source("register_global"), points, candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations, damping,
                                          min_weight, max_residual, Ts)

    def register_map_points_global(self, other, points, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10,
                                   damping=1e-3, min_weight=1, max_residual=0.9, Ts=None):
        """register_points_global against the map of `other` (another KinectFusion of this process, which is only read); T takes the points to ITS volume frame."""
        return self._register_global_call(self._source("register_global", other=other), points, candidates, keep, rounds, stride, box_t, refine_t, refine_r,
                                          iterations, damping, min_weight, max_residual, Ts)

    def register_checkpoint_points_global(self, path, points, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10,
                                          damping=1e-3, min_weight=1, max_residual=0.9, Ts=None):
        """register_points_global against the map in a checkpoint file of a whole volume (save_checkpoint, dense or sparse), validated as merge_checkpoint does."""
        return self._register_global_call(self._source("register_global", path=path), points, candidates, keep, rounds, stride, box_t, refine_t,
                                          refine_r, iterations, damping, min_weight, max_residual, Ts)

    def register_and_fuse(self, points, T0=None, origin=(0.0, 0.0, 0.0), iterations=10, damping=1e-3, min_weight=1, max_residual=0.9, min_range=0.2, max_range=5.0,
                          carve=False, weight=1, global_search=False):
        """register_points followed, when it succeeded, by fuse_points at the winning transform: (ok, T, register report, fuse counts or None).
        Nothing is fused when no start ended ok.  global_search=True: the registration is register_points_global at its defaults (with these
        iterations, damping, min_weight and max_residual) and T0 is not used; the report is that call's."""
        if global_search:
            ok, T, rep = self.register_points_global(points, iterations=iterations, damping=damping, min_weight=min_weight, max_residual=max_residual)
        else:
            ok, T, rep = self.register_points(points, T0, iterations, damping, min_weight, max_residual)
        fused = self.fuse_points(points, T, origin, min_range, max_range, carve, weight) if ok else None
        return ok, T, rep, fused

    def release_fuse_scratch(self):
        """Frees fuse_points' accumulator (8 bytes per voxel); the next fuse_points allocates it again."""
        _lib.xs_kf_release_fuse_scratch(self.h)

    def _score_transforms_call(self, source, Ts, stride, min_weight, max_residual, cloud=(), bad=""):
        name, fn, lead = source
        t = transform_stack(Ts)
        out = np.zeros((t.shape[0], 2), np.float64)
        rc = fn(*lead, *cloud[:3], t.shape[0], t.ctypes.data_as(_f64p), int(stride), int(min_weight), float(max_residual), out.ctypes.data_as(_f64p))
        _map_rc(name, rc, bad + _BAD_SEARCH)
        return out

    def score_transforms(self, other, Ts, stride=1, min_weight=1, max_residual=1.0):
        """{sum r^2, count} [P, 2] float64 of "the map of `other` resampled under T minus this map" over every stride-th voxel of this map's
        band, for each T of Ts [P, 4, 4] (as merge_map takes T), in one launch per 4096 transforms: the residual and the gates of align_map,
        without derivatives.  S = count - sum r^2 ranks the transforms.  Nothing is modified.  XsError in shard mode, ValueError on bad arguments."""
        return self._score_transforms_call(self._source("score_transforms", other=other), Ts, stride, min_weight, max_residual)

    def score_transforms_checkpoint(self, path, Ts, stride=1, min_weight=1, max_residual=1.0):
        """score_transforms with the other map read from a checkpoint file of a whole volume (either format is accepted), validated as merge_checkpoint does."""
        return self._score_transforms_call(self._source("score_transforms", path=path), Ts, stride, min_weight, max_residual)

    def _align_global_call(self, source, *search):
        """search: the search arguments, candidates .. Ts, as fill_search_opts takes them."""
        name, fn, lead = source
        o = AlignSearchOpts()
        _lib.xs_kf_align_search_defaults(self.h, C.byref(o))
        user = fill_search_opts(o, *search)   # (held until the call has returned)
        out, rep = np.eye(4, dtype=np.float64), np.zeros(12, np.float64)
        rc = fn(*lead, C.byref(o), out.ctypes.data_as(_f64p), rep.ctypes.data_as(_f64p))
        _map_rc(name, rc, _BAD_SEARCH, zero_ok=True)
        return rc == 1, out, report(rep, ALIGN_SEARCH_REPORT)

    def align_map_global(self, other, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10, damping=1e-3,
                         min_weight=1, max_residual=1.0, Ts=None):
        """align_map with no starting guess: `candidates` transforms that cover all rotations (transform_candidates_free; translations from the
        two maps' band centroids, jittered by box_t metres) are scored over every stride-th band voxel (score_transforms), the `keep` best by
        S = count - sum r^2 are refined over `rounds` rounds of candidates about each (transform_candidates_around: boxes refine_t metres and
        refine_r radians, halved per round), and the kept transforms start align_map's loop.  box_t, refine_t None: this map's truncation
        distance.  Ts [N, 4, 4]: candidates of the caller's that replace the free ones.  Returns (ok, T [4, 4] float64, report dict); ok False
        (T = the identity) when no start ended ok.  The score cannot tell a scene from its image under one of its own symmetries: a symmetric
        scene has several equally good answers and any of them may be returned.  Nothing is modified.  XsError in shard mode, ValueError on
        bad arguments.  Intended use: kf.merge_map(other, kf.align_map_global(other)[1])."""
        return self._align_global_call(self._source("align_global", other=other), candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations, damping,
                                       min_weight, max_residual, Ts)

    def align_checkpoint_global(self, path, candidates=2048, keep=8, rounds=2, stride=4, box_t=None, refine_t=None, refine_r=0.25, iterations=10, damping=1e-3,
                                min_weight=1, max_residual=1.0, Ts=None):
        """align_map_global with the other map read from a checkpoint file of a whole volume (save_checkpoint, dense or sparse: either format is accepted), validated as merge_checkpoint
        does.  Intended use: kf.merge_checkpoint(path, kf.align_checkpoint_global(path)[1])."""
        return self._align_global_call(self._source("align_global", path=path), candidates, keep, rounds, stride, box_t, refine_t, refine_r, iterations,
                                       damping, min_weight, max_residual, Ts)
