"""KinectFusion's methods of the tracking run itself: frames in, poses and maps out, relocalisation against the map, export, checkpoints,
and the profiling and debugging counters."""
import ctypes as C

import numpy as np

from .pipeline_abi import MAPS, STAGES, _f32p, _f64p, _i32p, _lib, _sz
from .pipeline_hostmath import Mesh, yaml_text
from .pipeline_marshal import RELOCALIZE_REPORT, check_rc, depth_pointers, pose_stack, report


class Handle:
    """What KinectFusion (C prefix xs_kf_) and ReferenceCallShape (xs_refshape_) share: both are handles on a C++ object that is made from
    the configuration text, fed frames and asked for poses, volume, maps and the ICP log; these entry points differ in the prefix alone."""
    _PREFIX, _ICP_LOG_COLUMNS = "xs_kf_", 55

    def _c(self, name):
        return getattr(_lib, self._PREFIX + name)

    def _open(self, params, failure):
        text = params if isinstance(params, str) else yaml_text(params)
        self.cfg = {}
        for line in text.splitlines():
            if ":" in line:
                k, v = line.split(":", 1)
                self.cfg[k.strip()] = v.split("#")[0].strip()
        self.h = self._c("create")(text.encode())
        if not self.h:
            raise ValueError(failure)
        self.res = [int(self.cfg[f"tsdf_size_{a}"]) for a in "xyz"]
        self.width, self.height = int(self.cfg["depth_width"]), int(self.cfg["depth_height"])

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            self._c("destroy")(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @property
    def frame_id(self):
        return self._c("frame_id")(self.h)

    def world2camera(self, idx=-1):
        out = np.zeros(32, np.float32)
        self._c("get_world2camera")(self.h, idx, out.ctypes.data_as(_f32p))
        return out.reshape(4, 4, 2)

    def icp_log(self):
        n = self._c("icp_log")(self.h, None, 0)
        out = np.zeros(n, np.float64)
        if n:
            self._c("icp_log")(self.h, out.ctypes.data_as(_f64p), n)
        return out.reshape(-1, self._ICP_LOG_COLUMNS)

    def volume(self):
        n = self.res[0] * self.res[1] * self.res[2]
        v, w, g = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        self._c("download_volume")(self.h, v.ctypes.data_as(_f32p), w.ctypes.data_as(_i32p), g.ctypes.data_as(_f32p))
        return v, w, g

    def map(self, which, level):
        rows, cols = self.height >> level, self.width >> level
        planes = 1 if which == "depths_curr" else 3
        out = np.zeros((planes * rows, cols, 2), np.float32)
        rc = self._c("download_map")(self.h, MAPS[which], level, out.ctypes.data_as(_f32p))
        assert rc == 0
        return out


class Tracking(Handle):
    """Mixin of KinectFusion (pipeline.py)."""

    def process_frame(self, depth_dev, step_bytes=None):
        """depth_dev: torch int16/uint16 CUDA tensor [H, W] (u16 millimetres) or a raw device address."""
        ptr = depth_dev if isinstance(depth_dev, int) else depth_dev.data_ptr()
        step = step_bytes if step_bytes is not None else self.width * 2
        return _lib.xs_kf_process_frame(self.h, ptr, step)

    def hint_next_frame(self, depth_dev, step_bytes=None):
        """The device depth image the NEXT process_frame call will be given (unchanged until then): its maps are built
        during this frame's ICP loop.  Call before process_frame of the current frame."""
        _lib.xs_kf_hint_next_frame(self.h, depth_dev.data_ptr(), step_bytes or self.width * 2)

    def process_frame_host(self, depth_u16):
        """Host frame [H, W] u16: staged through pinned memory and copied asynchronously on the second stream
        (an array returned by ingest_buffer() is used in place)."""
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        return _lib.xs_kf_process_frame_host(self.h, d.ctypes.data)

    def ingest_buffer(self):
        """The next host-pinned staging buffer as a [H, W] uint16 array: fill it, then process_frame_host(it)."""
        ptr = _lib.xs_kf_ingest_buffer(self.h)
        n = self.width * self.height
        return np.ctypeslib.as_array((C.c_uint16 * n).from_address(ptr)).reshape(self.height, self.width)

    def camera2volume(self):
        out = np.zeros(32, np.float32)
        _lib.xs_kf_get_camera2volume(self.h, out.ctypes.data_as(_f32p))
        return out.reshape(4, 4, 2)

    def gauss_newton_terms(self, depth_dev, c2v):
        """29 doubles: J^T J upper triangle (21), J^T r (6), sum r^2, count, for the residual of the depth frame
        against the map at camera2volume c2v [4, 4, 2]."""
        m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32)
        out = np.zeros(29, np.float64)
        ok = _lib.xs_kf_gauss_newton_terms(self.h, depth_dev.data_ptr(), self.width * 2, m.ctypes.data_as(_f32p), out.ctypes.data_as(_f64p))
        return out if ok == 1 else None

    def pose_hessian_terms(self, depth_dev, c2v):
        """29 doubles: H upper triangle (21), g (6), sum r^2, count — the exact Hessian and the gradient of L = sum r^2 in the twist of
        c2v <- se3Exp(theta) c2v, from one launch over the map's band index."""
        m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32)
        out = np.zeros(29, np.float64)
        ok = _lib.xs_kf_pose_hessian_terms(self.h, depth_dev.data_ptr(), self.width * 2, m.ctypes.data_as(_f32p), out.ctypes.data_as(_f64p))
        return out if ok == 1 else None

    def pose_hessian(self, depth_dev, c2v):
        """(H [6, 6] symmetric, g [6], sum r^2, count) of pose_hessian_terms."""
        s = self.pose_hessian_terms(depth_dev, c2v)
        if s is None:
            return None
        H = np.zeros((6, 6))
        H[np.triu_indices(6)] = s[:21]
        H = H + np.triu(H, 1).T
        return H, s[21:27].copy(), float(s[27]), int(s[28])

    def relocalize(self, depth_dev, c2v, iterations=5, damping=1e-3, method="gauss_newton"):
        """Refinement of camera2volume against the map: (ok, refined c2v [4, 4, 2], loss history).  method "gauss_newton" (first-order
        seeds) or "newton" (the exact Hessian; the return then gains the number of iterations that fell back to Gauss-Newton)."""
        m = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32).copy()
        hist = np.zeros(iterations + 1, np.float64)
        if method == "newton":
            fb = C.c_int(0)
            ok = _lib.xs_kf_relocalize_newton(self.h, depth_dev.data_ptr(), self.width * 2, m.ctypes.data_as(_f32p), iterations, damping,
                                              hist.ctypes.data_as(_f64p), C.cast(C.byref(fb), _i32p))
            return ok == 1, m.reshape(4, 4, 2), hist, int(fb.value)
        if method != "gauss_newton":
            raise ValueError(f"relocalize: unknown method {method!r}")
        ok = _lib.xs_kf_relocalize(self.h, depth_dev.data_ptr(), self.width * 2, m.ctypes.data_as(_f32p), iterations, damping,
                                   hist.ctypes.data_as(_f64p))
        return ok == 1, m.reshape(4, 4, 2), hist

    def relocalize_batch(self, depths, c2vs, iterations=5, damping=1e-3, method="gauss_newton"):
        """relocalize for F depth frames at once over the map's band index: (ok [F] bool, refined c2v [F, 4, 4, 2], loss histories
        [F, iterations + 1]; with method "newton" also the fallback counts [F]).  Frame f's results equal
        relocalize(depths[f], c2vs[f], ..., method=method) bit for bit."""
        F = len(depths)
        m = np.ascontiguousarray(c2vs, dtype=np.float32).reshape(F * 32).copy()
        hist = np.zeros((F, iterations + 1), np.float64)
        ok = np.zeros(F, np.int32)
        P = depth_pointers(depths)
        if method == "newton":
            fb = np.zeros(max(F, 1), np.int32)
            n = _lib.xs_kf_relocalize_newton_batch(self.h, F, P, self.width * 2, m.ctypes.data_as(_f32p), iterations, damping,
                                                   hist.ctypes.data_as(_f64p), ok.ctypes.data_as(_i32p), fb.ctypes.data_as(_i32p))
            if n < 0:
                raise ValueError("xs_kf_relocalize_newton_batch: bad arguments")
            return ok == 1, m.reshape(F, 4, 4, 2), hist, fb[:F]
        if method != "gauss_newton":
            raise ValueError(f"relocalize_batch: unknown method {method!r}")
        n = _lib.xs_kf_relocalize_batch(self.h, F, P, self.width * 2, m.ctypes.data_as(_f32p), iterations, damping, hist.ctypes.data_as(_f64p),
                                        ok.ctypes.data_as(_i32p))
        if n < 0:
            raise ValueError("xs_kf_relocalize_batch: bad arguments")
        return ok == 1, m.reshape(F, 4, 4, 2), hist

    def score_poses(self, depth_dev, c2vs):
        """The alignment loss of one depth frame at P camera2volume hypotheses c2vs [P, 4, 4, 2] in one pass over the map's band index per
        4096 poses: (sum loss [P], count [P]) float64 — per pose what xs_compute_local_tsdf_loss gives on the dense map."""
        m, P = pose_stack(c2vs)
        out = np.zeros((max(P, 1), 2), np.float64)
        rc = _lib.xs_kf_score_poses(self.h, depth_dev.data_ptr(), self.width * 2, P, m.ctypes.data_as(_f32p), out.ctypes.data_as(_f64p))
        check_rc("xs_kf_score_poses", rc, shard=None, bad_text="bad arguments", rest="bad arguments" if rc < 0 else "no volume")
        return out[:P, 0].copy(), out[:P, 1].copy()

    def relocalize_global(self, depth_dev, candidates, keep=8, iterations=10, damping=1e-3):
        """Global relocalisation from pose hypotheses candidates [P, 4, 4, 2] (pose_candidates makes them): score all, refine the `keep`
        with the highest S = count - sum loss by Gauss-Newton, return the refined pose with the highest S: (ok, c2v [4, 4, 2], report).
        Not ok (none of the kept converged): c2v is candidates[0] and the report's index is -1."""
        m, P = pose_stack(candidates)
        assert P > 0
        best = m[:32].copy()
        rep = np.zeros(8, np.float64)
        rc = _lib.xs_kf_relocalize_global(self.h, depth_dev.data_ptr(), self.width * 2, P, m.ctypes.data_as(_f32p), int(keep), int(iterations),
                                          float(damping), best.ctypes.data_as(_f32p), rep.ctypes.data_as(_f64p))
        if rc < 0:
            raise ValueError("xs_kf_relocalize_global: bad arguments")
        return rc == 1, best.reshape(4, 4, 2), report(rep, RELOCALIZE_REPORT)

    def relocalization_index_voxels(self):
        """Band voxels in the relocalisation index as last built by relocalize_batch (0 before the first)."""
        return int(_lib.xs_kf_relocalization_index_voxels(self.h))

    def export_point_cloud(self, max_buffer=1000000):
        """ExportPointCloud: (points [n, 3], normals [n, 3]) float32 on the host."""
        p = np.zeros((max_buffer, 3), np.float32)
        nr = np.zeros((max_buffer, 3), np.float32)
        n = _lib.xs_kf_export_point_cloud(self.h, max_buffer, p.ctypes.data_as(_f32p), nr.ctypes.data_as(_f32p))
        return p[:n], nr[:n]

    def export_ply(self, filename, max_buffer=1000000):
        return _lib.xs_kf_export_ply(self.h, max_buffer, str(filename).encode())

    def export_mesh(self, min_weight=1):
        """ExportMesh: the marching-cubes mesh on the host, a Mesh of vertices [V, 3] f32, vertex_im [V, 3] f32 (raw Im, divide by
        csfd_seed_h; None without a CSFD seed), normals [V, 3] f32, triangles [T, 3] i32 and edge_keys [V] u64."""
        nt, has_im = C.c_longlong(0), C.c_int(0)
        nv = _lib.xs_kf_export_mesh(self.h, min_weight, 0, 0, None, None, None, None, None, C.byref(nt), C.byref(has_im))
        while True:   # (the volume does not change between the calls: one retry)
            cap_v, cap_t = nv, nt.value
            v, n, im = (np.zeros((cap_v, 3), np.float32) for _ in range(3))
            k = np.zeros(cap_v, np.uint64)
            t = np.zeros((cap_t, 3), np.int32)
            nv = _lib.xs_kf_export_mesh(self.h, min_weight, cap_v, cap_t, v.ctypes.data_as(_f32p), n.ctypes.data_as(_f32p), im.ctypes.data_as(_f32p),
                                        k.ctypes.data_as(C.POINTER(C.c_uint64)), t.ctypes.data_as(_i32p), C.byref(nt), C.byref(has_im))
            if nv <= cap_v and nt.value <= cap_t:
                return Mesh(v[:nv], im[:nv] if has_im.value else None, n[:nv], t[:nt.value], k[:nv])

    def export_mesh_ply(self, filename):
        """Binary little-endian PLY of export_mesh (with dx dy dz = vertex_im while a CSFD seed is active); the vertex count, -1 on failure."""
        return _lib.xs_kf_export_mesh_ply(self.h, str(filename).encode())

    def synchronize(self):
        _lib.xs_kf_synchronize(self.h)

    def num_poses(self):
        return _lib.xs_kf_num_poses(self.h)

    def tranc_dist(self):
        return _lib.xs_kf_tranc_dist(self.h)

    def last_U(self):
        return _lib.xs_kf_last_updated_voxels(self.h)

    def last_hits(self):
        return _lib.xs_kf_last_raycast_hits(self.h)

    def volume_ptr(self, which):
        step = _sz(0)
        p = _lib.xs_kf_volume_ptr(self.h, {"value": 0, "weight": 1, "grad": 2}[which], C.byref(step))
        return p, step.value

    def set_profiling(self, level=2):
        """0 off, 1 integrate-kernel events + counters only, 2 (True) every stage."""
        _lib.xs_kf_set_profiling(self.h, 2 if level is True else int(level))

    def stage_times(self):
        ms = np.zeros(6, np.float64)
        calls = (C.c_longlong * 6)()
        _lib.xs_kf_stage_times(self.h, ms.ctypes.data_as(_f64p), calls)
        return {s: (float(ms[i]), int(calls[i])) for i, s in enumerate(STAGES)}

    def cumulative_counters(self):
        u, h = C.c_longlong(0), C.c_longlong(0)
        _lib.xs_kf_cumulative_counters(self.h, C.byref(u), C.byref(h))
        return u.value, h.value

    def reset_stage_times(self):
        _lib.xs_kf_reset_stage_times(self.h)

    def icp_iteration_times(self):
        """{slot: (microseconds summed, iterations)} of the ICP loop's host-side iteration period since the last reset; slots 0..2 = pyramid
        level, 3 = the first iteration of each frame (which also waits for the previous frame's tail)."""
        us = np.zeros(4, np.float64)
        calls = (C.c_longlong * 4)()
        _lib.xs_kf_icp_iteration_times(self.h, us.ctypes.data_as(_f64p), calls)
        return {lv: (float(us[lv]), int(calls[lv])) for lv in range(4)}

    def tail_host_times(self):
        """Mean host microseconds per frame of the tail's four host stretches since the last reset (xs_kf_tail_host_times)."""
        us = np.zeros(4, np.float64)
        n = C.c_longlong(0)
        _lib.xs_kf_tail_host_times(self.h, us.ctypes.data_as(_f64p), C.byref(n))
        k = max(int(n.value), 1)
        return {"frames": int(n.value), "sums_seen_to_integrate_entered": round(float(us[0]) / k, 2), "entered_to_launch_call": round(float(us[1]) / k, 2),
                "integrate_launch_call": round(float(us[2]) / k, 2), "launch_returned_to_raycast_launched": round(float(us[3]) / k, 2)}

    def gn_poll_times(self, reset=False):
        """Mean microseconds a Gauss-Newton kernel that was enqueued ahead waited for its poses (the device's own clock), and how many such passes."""
        pu, n = C.c_double(0), C.c_longlong(0)
        _lib.xs_kf_gn_poll_times(self.h, C.byref(pu), C.byref(n), int(reset))
        return {"passes": int(n.value), "wait_us": pu.value / max(n.value, 1)}

    def set_gn_post_pose(self, on):
        _lib.xs_kf_set_gn_post_pose(self.h, int(bool(on)))

    def gn_times(self, reset=False):
        """Gauss-Newton passes run by relocalize since the last reset: mean wall clock per pass and (profiling on) mean kernel duration, microseconds."""
        pu, km = C.c_double(0), C.c_double(0)
        n, kc = C.c_longlong(0), C.c_longlong(0)
        _lib.xs_kf_gn_times(self.h, C.byref(pu), C.byref(n), C.byref(km), C.byref(kc), int(reset))
        return {"passes": int(n.value), "pass_us": pu.value / max(n.value, 1), "kernel_calls": int(kc.value), "kernel_us": 1e3 * km.value / max(kc.value, 1)}

    def debug_set_icp_sequence(self, v):
        _lib.xs_kf_debug_set_icp_sequence(self.h, int(v))

    def debug_fail_icp_iteration(self, n):
        _lib.xs_kf_debug_fail_icp_iteration(self.h, int(n))

    def debug_post_delay(self, min_us, max_us):
        """Test aid: a random host sleep of [min_us, max_us] microseconds in front of every ICP pose post."""
        _lib.xs_kf_debug_post_delay(self.h, int(min_us), int(max_us))

    def composite_bytes(self):
        """Shard mode: bytes this rank received through the raycast composite's collectives so far (see xs_kf_composite_bytes)."""
        return int(_lib.xs_kf_composite_bytes(self.h))

    def list_cover_counts(self):
        """Frames whose list / box classes decided ahead held for the final pose: {"neither": n, "list_only": n, "both": n}."""
        c = (C.c_longlong * 4)()
        _lib.xs_kf_list_cover_counts(self.h, c)
        return {"neither": int(c[0]), "list_only": int(c[1]), "both": int(c[3])}

    def rebuild_sign_map(self):
        """After writing the value array through volume_ptr: the ray march's sign map is rebuilt from the volume."""
        _lib.xs_kf_rebuild_sign_map(self.h)

    def volume_generation(self):
        """The version of the volume's contents: moves with every write of the volume, stays under calls that only read the map."""
        return int(_lib.xs_kf_volume_generation(self.h))

    def save_checkpoint(self, path, sparse=False):
        """The volume and the pose record to a file.  sparse=False: the dense XSTSDF2 dump, 12 bytes per voxel.  sparse=True: the brick-sparse
        XSTSDF3 (lossless; classified and compacted on the GPU, streamed through one pinned staging buffer), and the save's statistics as a dict:
        bricks, classes (bricks per class 0 .. 7), payload_words, file_bytes, chunks.  load_checkpoint and every *_checkpoint method take
        either file.  A rank of a sharded run saves its own planes in either format."""
        if not sparse:
            _lib.xs_kf_save_checkpoint(self.h, path.encode())
            return None
        s = (C.c_ulonglong * 12)()
        if _lib.xs_kf_save_checkpoint_sparse(self.h, path.encode(), s) != 0:
            raise OSError(f"save_checkpoint: cannot write {path}")
        return dict(bricks=int(s[0]), classes=[int(s[1 + c]) for c in range(8)], payload_words=int(s[9]), file_bytes=int(s[10]), chunks=int(s[11]))

    def checkpoint_staging_words(self, words=0):
        """The staging buffer of sparse saves and loads in 32-bit words (default 16 Mi = 64 MiB): set when words >= 1536, returned either way."""
        n = int(_lib.xs_kf_checkpoint_staging_words(self.h, int(words)))
        if n < 0:
            raise ValueError("checkpoint_staging_words: at least 1536 words (one brick at its largest)")
        return n

    def load_checkpoint(self, path):
        """Restores the volume, the pose record and the frame number from a checkpoint of either format (the magic decides), written by an
        instance of the same geometry (and, in shard mode, the same rank).  False, with the state unchanged, for any other file."""
        return _lib.xs_kf_load_checkpoint(self.h, path.encode()) == 0

    def save_tsdf_volume(self, path):
        _lib.xs_kf_save_tsdf_volume(self.h, path.encode())
