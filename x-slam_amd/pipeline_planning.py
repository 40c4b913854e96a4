"""KinectFusion's planning methods, which read the map and change nothing: what candidate views would see, clearance, reachability and
travel cost, paths, frontier clusters, and the views proposed from them."""
import ctypes as C

import numpy as np

from . import capi
from .pipeline_abi import _f32p, _i32p, _lib
from .pipeline_marshal import check_rc, optional, pose_stack, ptr, retry_capacity

# why each group of calls refuses shard mode
_VIEW = "occlusion along a ray is not additive over z-slabs"
_REACH = "distance and connectivity are not additive over z-slabs"
_FRONTIER = "neither connectivity nor a cluster is additive over z-slabs"


def _view_query(poses, rays, t_near, t_far, step, min_hits=0):
    """What the four view calls share: (flat poses, P, the counts [P, 4] to fill, the view options, min_hits or for None a quarter of the rays)."""
    m, P = pose_stack(poses)
    if min_hits is None:
        min_hits = int(rays[0]) * int(rays[1]) // 4
    return m, P, np.zeros((max(P, 1), 4), np.uint32), capi.view_opts(rays, t_near, t_far, step), min_hits


class Planning:
    """Mixin of KinectFusion (pipeline.py), which provides h, cfg and res."""

    def score_views(self, c2vs, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, min_weight=1):
        """What the camera would see from P hypothetical camera2volume poses c2vs [P, 4, 4, 2] (real parts; pose_candidates makes them), one
        launch over the volume's two-bit observation grid per 4096 poses: uint32 [P, 4] = {unknown, free, hits, frontier} samples per pose
        along rays[0] x rays[1] rays, depths t_near .. t_far in increments of `step` (None: a voxel).  XsError in shard mode."""
        m, P, out, opts, _ = _view_query(c2vs, rays, t_near, t_far, step)
        rc = _lib.xs_kf_score_views(self.h, P, m.ctypes.data_as(_f32p), C.byref(opts), int(min_weight), out.ctypes.data_as(C.POINTER(C.c_uint)))
        check_rc("xs_kf_score_views", rc, _VIEW, rest="no volume")
        return out[:P].copy()

    def next_best_view(self, candidates, min_hits=None, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, min_weight=1):
        """The candidate ([P, 4, 4, 2]) that sees the most unknown space among those with at least min_hits rays ending on a known surface
        (None: a quarter of the rays): (index, counts uint32 [P, 4] as score_views returns them); index -1 when no candidate qualifies.
        XsError in shard mode."""
        m, P, out, opts, min_hits = _view_query(candidates, rays, t_near, t_far, step, min_hits)
        rc = _lib.xs_kf_next_best_view(self.h, P, m.ctypes.data_as(_f32p), C.byref(opts), int(min_weight), int(min_hits),
                                       out.ctypes.data_as(C.POINTER(C.c_uint)))
        check_rc("xs_kf_next_best_view", rc, _VIEW, bad=-3, rest_ok=True)
        return int(rc), out[:P].copy()

    def clearance_field(self, max_radius_vox=8, unknown_blocks=True, min_weight=1):
        """How far the nearest obstacle is: uint16 [Z, Y, X] = min(d^2, R^2) in voxels, R = max_radius_vox (1 .. 255), to the nearest OCCUPIED
        voxel — with unknown_blocks also the nearest UNKNOWN voxel or position outside the volume — of the observation grid at min_weight.
        XsError in shard mode."""
        out = np.zeros((self.res[2], self.res[1], self.res[0]), np.uint16)
        rc = _lib.xs_kf_clearance_field(self.h, int(max_radius_vox), int(bool(unknown_blocks)), int(min_weight), out.ctypes.data_as(C.POINTER(C.c_uint16)))
        check_rc("xs_kf_clearance_field", rc, _REACH, rest="no volume")
        return out

    def reachable(self, c2vs, radius_m, start=None, snap_vox=4, unknown_blocks=True, min_weight=1):
        """Which of the P camera2volume poses c2vs [P, 4, 4, 2] a body of radius_m can get to from `start` ([4, 4, 2]; None: the current
        camera2volume) through known free space: (reachable bool [P], clear2 uint16 [P] — the clearance field at each pose's centre voxel,
        squared voxels, capped at the R the radius needs).  The start is snapped to the nearest passable voxel within snap_vox voxels; the
        candidates are not snapped.  XsError in shard mode."""
        m, P = pose_stack(c2vs)
        flags, clear2 = np.zeros(max(P, 1), np.uint8), np.zeros(max(P, 1), np.uint16)
        s = optional(start, 32)
        rc = _lib.xs_kf_reachable(self.h, ptr(s, _f32p), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                                  int(min_weight), P, m.ctypes.data_as(_f32p), flags.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                  clear2.ctypes.data_as(C.POINTER(C.c_uint16)))
        check_rc("xs_kf_reachable", rc, _REACH, rest="no volume")
        return flags[:P].astype(bool), clear2[:P].copy()

    def next_reachable_view(self, candidates, radius_m, min_hits=None, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, min_weight=1, snap_vox=4,
                            unknown_blocks=True):
        """next_best_view among the candidates a body of radius_m can get to from the current camera through known free space: (index, counts
        uint32 [P, 4], reachable bool [P]); index -1 when no reachable candidate qualifies.  XsError in shard mode."""
        m, P, out, opts, min_hits = _view_query(candidates, rays, t_near, t_far, step, min_hits)
        flags = np.zeros(max(P, 1), np.uint8)
        rc = _lib.xs_kf_next_reachable_view(self.h, P, m.ctypes.data_as(_f32p), C.byref(opts), int(min_weight), int(min_hits),
                                            out.ctypes.data_as(C.POINTER(C.c_uint)), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                                            flags.ctypes.data_as(C.POINTER(C.c_ubyte)))
        check_rc("xs_kf_next_reachable_view", rc, _REACH, bad=-3, rest_ok=True)
        return int(rc), out[:P].copy(), flags[:P].astype(bool)

    def _travel_m(self, units):
        """uint16 travel costs (thirds of a voxel edge) as float64 metres, inf for 65535."""
        vs = float(np.float32(float(self.cfg["tsdf_voxel_size"])))
        u = np.asarray(units, np.uint16)
        return np.where(u == capi.TRAVEL_NONE, np.inf, u.astype(np.float64) * vs / 3.0)

    def travel(self, c2vs, radius_m, start=None, snap_vox=4, unknown_blocks=True, min_weight=1, max_travel_m=None):
        """reachable() plus how far each pose is: (reachable bool [P], clear2 uint16 [P], travel_m float64 [P]) — the length in metres of the
        shortest path of 26-neighbour moves that cuts no corner (the <3, 4, 5> chamfer metric) from the snapped start to each pose's centre
        voxel through the reached voxels, inf where unreachable or beyond max_travel_m (None: no limit but 65534 thirds of a voxel).
        XsError in shard mode."""
        m, P = pose_stack(c2vs)
        flags, clear2, cost = np.zeros(max(P, 1), np.uint8), np.zeros(max(P, 1), np.uint16), np.zeros(max(P, 1), np.uint16)
        s = optional(start, 32)
        rc = _lib.xs_kf_travel(self.h, ptr(s, _f32p), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                               int(min_weight), 0.0 if max_travel_m is None else float(max_travel_m), P, m.ctypes.data_as(_f32p),
                               flags.ctypes.data_as(C.POINTER(C.c_ubyte)), clear2.ctypes.data_as(C.POINTER(C.c_uint16)),
                               cost.ctypes.data_as(C.POINTER(C.c_uint16)))
        check_rc("xs_kf_travel", rc, _REACH, rest="no volume")
        return flags[:P].astype(bool), clear2[:P].copy(), self._travel_m(cost[:P])

    def path_to(self, c2v, radius_m, start=None, snap_vox=4, unknown_blocks=True, min_weight=1, max_travel_m=None, capacity=1024):
        """The shortest collision-free path from the snapped start to the centre voxel of pose c2v ([4, 4, 2]), start first and target last:
        (points float32 [n, 3] — the voxel centres in volume coordinates, metres —, voxels int32 [n, 3]), or None when the target is not
        reached (or beyond max_travel_m).  A path longer than `capacity` voxels is fetched by one more call.  XsError in shard mode."""
        t = np.ascontiguousarray(c2v, dtype=np.float32).reshape(32)
        s = optional(start, 32)

        def run(capacity):
            voxels, points, needed = np.zeros((capacity, 3), np.int32), np.zeros((capacity, 3), np.float32), C.c_int(0)
            rc = _lib.xs_kf_path_to(self.h, ptr(s, _f32p), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                                    int(min_weight), 0.0 if max_travel_m is None else float(max_travel_m), t.ctypes.data_as(_f32p), capacity,
                                    voxels.ctypes.data_as(_i32p), points.ctypes.data_as(_f32p), C.byref(needed))
            return rc, int(needed.value), (voxels, points)

        rc, (voxels, points) = retry_capacity(run, max(int(capacity), 1))
        check_rc("xs_kf_path_to", rc, _REACH, rest_ok=True)
        if rc < 0:
            raise capi.XsError(f"xs_kf_path_to: {rc}")
        return None if rc == 0 else (points[:rc].copy(), voxels[:rc].copy())

    def next_view_by_travel(self, candidates, radius_m, bias_m=0.5, min_hits=None, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, min_weight=1,
                            snap_vox=4, unknown_blocks=True, max_travel_m=None):
        """Weighs what a view sees against how far away it is: among the candidates a body of radius_m can get to from the current camera
        (within max_travel_m) with at least min_hits rays on a known surface, the one with the largest unknown / (travel + bias), bias_m
        being the fixed cost of taking any view at all: (index, counts uint32 [P, 4], travel_m float64 [P]); index -1 when no candidate
        qualifies.  XsError in shard mode."""
        m, P, out, opts, min_hits = _view_query(candidates, rays, t_near, t_far, step, min_hits)
        cost = np.zeros(max(P, 1), np.uint16)
        rc = _lib.xs_kf_next_view_by_travel(self.h, P, m.ctypes.data_as(_f32p), C.byref(opts), int(min_weight), int(min_hits),
                                            out.ctypes.data_as(C.POINTER(C.c_uint)), float(radius_m), int(snap_vox), int(bool(unknown_blocks)),
                                            0.0 if max_travel_m is None else float(max_travel_m), float(bias_m), cost.ctypes.data_as(C.POINTER(C.c_uint16)))
        check_rc("xs_kf_next_view_by_travel", rc, _REACH, bad=-3, rest_ok=True)
        return int(rc), out[:P].copy(), self._travel_m(cost[:P])

    FRONTIER_DTYPE = np.dtype([("label", np.uint32), ("count", np.uint64), ("sum", np.uint64, 3), ("centroid", np.float32, 3), ("min", np.int32, 3),
                               ("max", np.int32, 3)])

    def frontiers(self, cell_vox=32, min_size=8, min_weight=1):
        """Where known free space borders the unknown, grouped: the clusters of the frontier voxels (FREE with an UNKNOWN face neighbour in the
        observation grid at min_weight; 26-adjacency within cells of cell_vox voxels, 0: the whole volume, otherwise a multiple of 8) that
        have at least min_size voxels, in ascending label order.  A structured array with fields label (the lowest linear voxel index
        (z Y + y) X + x of the cluster), count, sum (of x, y, z), centroid (float32 metres in volume coordinates: (sum / count + 0.5) voxels)
        and the bounding box min / max (x, y, z voxels, inclusive).  XsError in shard mode."""
        n = C.c_int(0)

        def run(capacity):
            rec = np.zeros((max(capacity, 1), capi.FRONTIER_RECORD_WORDS), np.uint64)
            rc = _lib.xs_kf_frontiers(self.h, int(cell_vox), int(min_size), int(min_weight), capacity, rec.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n))
            return rc, int(n.value), rec

        rc, rec = retry_capacity(run, 1024)
        check_rc("xs_kf_frontiers", rc, _FRONTIER)
        return self._cluster_records(rec[:n.value])

    def _cluster_records(self, rec):
        """Records of 8 uint64 in the frontier's format [n, 8] as a structured array of FRONTIER_DTYPE: label, count, sum, the centroid in
        metres and the bounding box."""
        out = np.zeros(len(rec), self.FRONTIER_DTYPE)
        out["label"], out["count"], out["sum"] = rec[:, 0], rec[:, 1], rec[:, 2:5]
        vs = np.float32(float(self.cfg["tsdf_voxel_size"]))
        q = (rec[:, 2:5].astype(np.float64) / np.maximum(rec[:, 1:2], 1).astype(np.float64)).astype(np.float32)
        out["centroid"] = (q + np.float32(0.5)) * vs
        for name, col in (("min", 5), ("max", 6)):
            out[name] = np.stack([(rec[:, col] >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32)], axis=1).astype(np.int32)
        return out

    def propose_views(self, radius_m, views_per_cluster=6, standoff_m=1.0, cell_vox=32, min_size=8, snap_vox=4, start_snap_vox=4, unknown_blocks=True,
                      min_weight=1):
        """Candidate views from the map alone: for every cluster frontiers(cell_vox, min_size, min_weight) returns, views_per_cluster
        standpoints at standoff_m around its centroid (Halton directions), each snapped to the nearest voxel within snap_vox that a body of
        radius_m reaches from the current camera (its start snapped within start_snap_vox, as reachable() does), duplicates and
        standpoints with no such voxel dropped: (c2vs float32 [P, 4, 4, 2] — at the voxel's centre, looking at the centroid —, cluster index
        int32 [P] into that list).  reachable() and travel() call every proposed pose reachable.  XsError in shard mode."""
        n = C.c_int(0)

        def run(capacity):
            m, idx = np.zeros((max(capacity, 1), 4, 4, 2), np.float32), np.zeros(max(capacity, 1), np.int32)
            rc = _lib.xs_kf_propose_views(self.h, float(radius_m), int(start_snap_vox), int(bool(unknown_blocks)), int(min_weight), int(cell_vox), int(min_size),
                                          int(views_per_cluster), float(standoff_m), int(snap_vox), capacity, m.ctypes.data_as(_f32p), idx.ctypes.data_as(_i32p),
                                          C.byref(n))
            return rc, int(n.value), (m, idx)

        rc, (m, idx) = retry_capacity(run, 1024)
        check_rc("xs_kf_propose_views", rc, _FRONTIER)
        return m[:n.value].copy(), idx[:n.value].copy()

    def explore_step(self, radius_m, views_per_cluster=6, standoff_m=1.0, cell_vox=32, min_size=8, snap_vox=4, unknown_blocks=True, min_weight=1, bias_m=0.5,
                     min_hits=None, rays=(80, 60), t_near=0.2, t_far=5.0, step=None, max_travel_m=None):
        """Where should the camera go next, and which way?  propose_views, then next_view_by_travel over the proposed poses, then path_to the
        chosen one (the start is snapped within snap_vox in all three).  A dict with index (into propose_views' list for the same arguments),
        pose [4, 4, 2], cluster, counts uint32 [4] = {unknown, free, hits, frontier}, travel_m and path (path_to's (points, voxels)); None
        when no view is proposed or none qualifies.  XsError in shard mode."""
        cands, cluster = self.propose_views(radius_m, views_per_cluster, standoff_m, cell_vox, min_size, snap_vox, snap_vox, unknown_blocks, min_weight)
        if len(cands) == 0:
            return None
        pick, counts, travel_m = self.next_view_by_travel(cands, radius_m, bias_m=bias_m, min_hits=min_hits, rays=rays, t_near=t_near, t_far=t_far, step=step,
                                                          min_weight=min_weight, snap_vox=snap_vox, unknown_blocks=unknown_blocks, max_travel_m=max_travel_m)
        if pick < 0:
            return None
        path = self.path_to(cands[pick], radius_m, snap_vox=snap_vox, unknown_blocks=unknown_blocks, min_weight=min_weight, max_travel_m=max_travel_m)
        return dict(index=pick, pose=cands[pick].copy(), cluster=int(cluster[pick]), counts=counts[pick].copy(), travel_m=float(travel_m[pick]), path=path)
