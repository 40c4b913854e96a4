"""Multi-GPU driver: one process per GPU, the TSDF volume sharded by z-slab, ICP by pixel rows
(the reference itself is single-GPU).  The per-frame logic is the C++
orchestrator in shard mode (x-slam_amd/host/KinectFusionReconstruction.cpp); this module only
supplies the collectives it calls back into, over torch.distributed (backend "nccl" = RCCL over
xGMI on the GPU box):

  op 0  sum of 55 doubles      — the 27 complex<double> ICP normal-equation sums + inlier count,
                                 once per ICP iteration (440 bytes, latency-bound)
  op 1  min of W*H int32       — first raycast event along every ray
  op 2  sum of int32           — the ranks' owned-pixel counts (one non-zero entry per rank); with shard_composite_gather: false the
                                 vertex / normal maps as bit patterns, only the owning rank non-zero
  op 3  gather of variable parts — the ranks' packed owned pixels (52 bytes each: pixel index, vertex, normal), each rank's part at the
                                 offset every rank derives from the counts: one broadcast per rank (a ring all-reduce of the maps moves
                                 every pixel's 48 bytes twice; this moves each owned pixel's 52 bytes once)

No volume data ever crosses ranks: halo planes are integrated redundantly by both neighbours
(the update is per voxel and deterministic, so the bits agree).
"""
import ctypes as C
import threading

import numpy as np

from . import pipeline as pl

HALO = 6  # planes each side; KinectFusionReconstruction::HALO

_CB = pl.COLLECTIVE_CB

OP_SUM_F64, OP_MIN_I32, OP_SUM_I32, OP_GATHERV = 0, 1, 2, 3
_TYPESTR = {OP_SUM_F64: "<f8", OP_MIN_I32: "<i4", OP_SUM_I32: "<i4"}


def slab_bounds(rank, world, Z, halo=HALO):
    """(owned z0, z1), (stored z0, z1) of a rank — the same arithmetic as the C++ side."""
    z0, z1 = Z * rank // world, Z * (rank + 1) // world
    if world == 1:
        return (z0, z1), (0, Z)
    return (z0, z1), (max(0, z0 - halo), min(Z, z1 + halo))


def row_bounds(rank, world, rows):
    return rows * rank // world, rows * (rank + 1) // world


def gatherv_descriptor(ptr, world):
    """(device buffer address, [byte offset of rank r's part for r = 0 .. world]) from the host array the orchestrator hands op 3."""
    words = (C.c_longlong * (world + 2)).from_address(int(ptr))
    return int(words[0]), [int(words[1 + r]) for r in range(world + 1)]


def gatherv_tensor(dist, torch, buf, offsets):
    """Every rank's part of the uint8 tensor `buf` (rank r's bytes offsets[r] .. offsets[r + 1]) to every rank: one broadcast per part."""
    for r in range(len(offsets) - 1):
        if offsets[r + 1] > offsets[r]:
            dist.broadcast(buf[offsets[r]:offsets[r + 1]], src=r)
    return buf


def reduce_tensor(dist, op, t):
    """In-place all-reduce of a tensor over the default process group (nccl on GPUs, gloo in the
    CPU tests)."""
    dist.all_reduce(t, op=dist.ReduceOp.MIN if op == OP_MIN_I32 else dist.ReduceOp.SUM)
    return t


class _DevView:
    """Zero-copy view of device memory the C++ side owns, for torch.as_tensor."""

    def __init__(self, ptr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": typestr, "data": (int(ptr), False), "version": 2}


def device_tensor(torch, ptr, count, op):
    return torch.as_tensor(_DevView(ptr, count, _TYPESTR[op]), device="cuda")


class LocalWorld:
    """All ranks inside one process, one Python thread per rank, sharing one GPU and one stream.
    Used to exercise the sharded C++ path on a single-GPU box (tests); the collectives meet at a
    barrier and are computed with torch ops on the shared stream."""

    def __init__(self, torch, world):
        self.torch, self.world = torch, world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world

    def collective_for(self, rank):
        def cb(_user, op, ptr, count):
            if op == OP_GATHERV:
                base, off = gatherv_descriptor(ptr, count)
                t = self.torch.as_tensor(_DevView(base, max(off[-1], 1), "|u1"), device="cuda")
                self.slots[rank] = t
                self.barrier.wait()
                for r in range(count):          # every rank copies every other rank's part out of that rank's buffer
                    if r != rank and off[r + 1] > off[r]:
                        t[off[r]:off[r + 1]].copy_(self.slots[r][off[r]:off[r + 1]])
                self.torch.cuda.synchronize()
                self.barrier.wait()
                return
            t = device_tensor(self.torch, ptr, count, op)
            self.slots[rank] = t
            self.barrier.wait()
            if rank == 0:
                stack = self.torch.stack(self.slots)
                red = stack.min(dim=0).values if op == OP_MIN_I32 else stack.sum(dim=0)
                for s in self.slots:
                    s.copy_(red)
            self.barrier.wait()
        return cb


_rccl_lib = None


def rccl_lib():
    """libxslam_rccl.so (include/xslam_amd_rccl.h): the same three collectives as C++ RCCL calls."""
    global _rccl_lib
    if _rccl_lib is None:
        import os
        lib = C.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libxslam_rccl.so"))
        lib.xs_rccl_get_unique_id.restype = C.c_int
        lib.xs_rccl_get_unique_id.argtypes = [C.c_void_p]
        lib.xs_rccl_comm_create.restype = C.c_void_p
        lib.xs_rccl_comm_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        lib.xs_rccl_set_stream.restype = None
        lib.xs_rccl_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        lib.xs_rccl_comm_destroy.restype = C.c_int
        lib.xs_rccl_comm_destroy.argtypes = [C.c_void_p]
        lib.xs_rccl_all_reduce.restype = C.c_int
        lib.xs_rccl_all_reduce.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_long]
        lib.xs_rccl_version.restype = C.c_int
        lib.xs_rccl_last_error.restype = C.c_char_p
        _rccl_lib = lib
    return _rccl_lib


class NativeRccl:
    """An RCCL communicator owned by the C++ side.  The 128-byte unique id travels from rank 0 over an existing
    torch.distributed group (any backend) — after that no collective of the pipeline passes through Python: the
    orchestrator calls xs_rccl_collective directly."""

    def __init__(self, rank, world, dist=None, stream=None):
        lib = rccl_lib()
        buf = (C.c_ubyte * 128)()
        if rank == 0:
            if lib.xs_rccl_get_unique_id(buf) != 0:
                raise RuntimeError(lib.xs_rccl_last_error().decode())
        if world > 1:
            box = [bytes(buf)]
            dist.broadcast_object_list(box, src=0)
            buf = (C.c_ubyte * 128).from_buffer_copy(box[0])
        sp = None if stream is None else (stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream))
        self.handle = lib.xs_rccl_comm_create(buf, rank, world, sp)
        if not self.handle:
            raise RuntimeError(lib.xs_rccl_last_error().decode())
        self.callback = C.cast(lib.xs_rccl_collective, _CB)      # the C function itself, not a Python trampoline
        self.version = lib.xs_rccl_version()

    def all_reduce(self, op, tensor):
        rc = rccl_lib().xs_rccl_all_reduce(self.handle, op, tensor.data_ptr(), tensor.numel())
        if rc != 0:
            raise RuntimeError(rccl_lib().xs_rccl_last_error().decode())

    def close(self):
        if self.handle:
            rccl_lib().xs_rccl_comm_destroy(self.handle)
            self.handle = None


class ShardedKinectFusion(pl.KinectFusion):
    """One rank's shard of the pipeline.  `dist` is torch.distributed with an initialised process
    group, or pass `collective` (a Python callable (user, op, ptr, count)) directly.  score_views and next_best_view raise XsError on a
    shard and do nothing: occlusion along a ray is not additive over z-slabs; so do clearance_field, reachable and
    next_reachable_view: distance and connectivity are not additive either (section 4.19); and travel, path_to and next_view_by_travel: a path
    is not additive either (section 4.20); and frontiers, propose_views and explore_step: a cluster that crosses a slab border is not the
    union of the slabs' clusters (section 4.21)."""

    def __init__(self, params, rank, world, dist=None, collective=None, torch=None, native=None):
        text = params if isinstance(params, str) else pl.yaml_text(params)
        self.cfg = {}
        for line in text.splitlines():
            if ":" in line:
                k, v = line.split(":", 1)
                self.cfg[k.strip()] = v.split("#")[0].strip()
        self.rank, self.world = rank, world
        user = None
        if native is not None:
            # a NativeRccl communicator: the orchestrator calls the C++ collective with the comm handle as user data
            self._cb, user = native.callback, native.handle
        elif collective is None:
            if torch is None:
                import torch
            self._torch, self._dist = torch, dist

            views = {}  # (ptr, count, op) -> tensor view: the orchestrator's buffers are persistent, so the
                        # per-call cost of wrapping a raw pointer (tens of microseconds) is paid once

            def collective(_user, op, ptr, count):
                if op == OP_GATHERV:
                    base, off = gatherv_descriptor(ptr, count)
                    key = (base, -1, OP_GATHERV)
                    t = views.get(key)
                    if t is None:     # the whole gather buffer (the orchestrator allocates it once: room for every pixel)
                        # (entry size from the library, not a literal: xs_raycast_compose_entry_bytes.  Stream ordering: the orchestrator's
                        # copy of this rank's own part into the buffer is enqueued on the stream torch.distributed orders its collectives
                        # against — the current stream, which the pipeline was created on; a pipeline on another stream must synchronise first)
                        from . import capi as _capi
                        t = views[key] = self._torch.as_tensor(_DevView(base, self.width * self.height * _capi.raycast_compose_entry_bytes(), "|u1"), device="cuda")
                    gatherv_tensor(self._dist, self._torch, t, off)
                    return
                key = (int(ptr), int(count), int(op))
                t = views.get(key)
                if t is None:
                    t = views[key] = device_tensor(self._torch, ptr, count, op)
                reduce_tensor(self._dist, op, t)
        if native is None:
            self._cb = _CB(collective)  # keep the trampoline alive as long as the handle
        self.h = pl._lib.xs_kf_create_sharded(text.encode(), rank, world, self._cb, user)
        if not self.h:
            raise ValueError("xs_kf_create_sharded failed")
        self.res = [int(self.cfg[f"tsdf_size_{a}"]) for a in "xyz"]
        self.width, self.height = int(self.cfg["depth_width"]), int(self.cfg["depth_height"])
        o, s = (C.c_int * 2)(), (C.c_int * 2)()
        pl._lib.xs_kf_shard_planes(self.h, o, s)
        self.owned, self.stored = (o[0], o[1]), (s[0], s[1])
        assert (self.owned, self.stored) == slab_bounds(rank, world, self.res[2])

    def volume(self):
        """(value, weight, grad) of the planes this rank stores, dense, plane self.stored[0] first."""
        n = self.res[0] * self.res[1] * (self.stored[1] - self.stored[0])
        v, w, g = np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
        pl._lib.xs_kf_download_volume(self.h, v.ctypes.data_as(pl._f32p), w.ctypes.data_as(pl._i32p), g.ctypes.data_as(pl._f32p))
        return v, w, g

    def owned_volume(self):
        v, w, g = self.volume()
        a = (self.owned[0] - self.stored[0]) * self.res[0] * self.res[1]
        b = (self.owned[1] - self.stored[0]) * self.res[0] * self.res[1]
        return v[a:b], w[a:b], g[a:b]


def weld_meshes(meshes):
    """One mesh from the ranks' export_mesh results, in rank order: the vertices merged by edge key (a vertex on a plane two ranks share
    carries the same bits in both), the triangles concatenated (each rank meshes the cubes of its own planes) and re-indexed.  Works
    for any list of pl.Mesh whose cube planes are disjoint and ascending."""
    keys = np.concatenate([m.edge_keys for m in meshes])
    uniq, first = np.unique(keys, return_index=True)
    pick = lambda f: None if any(getattr(m, f) is None for m in meshes) else np.concatenate([getattr(m, f) for m in meshes])[first]
    tris = [np.searchsorted(uniq, m.edge_keys[m.triangles]).astype(np.int32) if len(m.triangles) else np.zeros((0, 3), np.int32)
            for m in meshes]
    return pl.Mesh(pick("vertices"), pick("vertex_im"), pick("normals"), np.concatenate(tris).reshape(-1, 3), uniq)


def tsdf_hessian_sharded(dist, rank, world, depth_scaled, scaled_step, rows, cols, intr, res, voxel_size, Rv2c, tv2c, tranc_dist, gt_slab,
                         workspace, out4, stream=None):
    """BASELINE config 4: the dual-complex Hessian kernel on this rank's z-slab of the ground-truth
    TSDF (gt_slab: dense planes [z0, z1) of the slab_bounds(rank, world, Z) owned range), then one
    all-reduce of the four sums {loss, grad, hessian, count}.  out4: 4-double CUDA tensor."""
    from . import capi
    (z0, z1), _ = slab_bounds(rank, world, int(res[2]))
    capi.compute_local_tsdf_hessian(depth_scaled, scaled_step, rows, cols, intr, res, voxel_size, Rv2c, tv2c, tranc_dist, gt_slab,
                                    workspace, out4, z0=z0, z1=z1, stream=stream)
    if world > 1:
        reduce_tensor(dist, OP_SUM_F64, out4)
    return out4
