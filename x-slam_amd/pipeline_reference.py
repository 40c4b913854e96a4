"""The test handle on the reference's own call shape: ReferenceCallShape, and the reference-signature TSDF loss and Hessian launchers."""
import numpy as np

from .pipeline_abi import _f32p, _i32p, _lib
from .pipeline_tracking import Handle


class ReferenceCallShape(Handle):
    """Handle to a C++ ReferenceCallShape (x-slam_amd/host/reference_shape.hpp): the reference's own per-frame call
    sequence over the reference-signature launchers alone, a stream drain where the reference drains the device."""

    _PREFIX, _ICP_LOG_COLUMNS = "xs_refshape_", 54

    def __init__(self, params):
        self._open(params, "xs_refshape_create failed (missing config key?)")

    def process_frame(self, depth_dev, step_bytes=None):
        ptr = depth_dev if isinstance(depth_dev, int) else depth_dev.data_ptr()
        return _lib.xs_refshape_process_frame(self.h, ptr, step_bytes if step_bytes is not None else self.width * 2)

    def process_frame_host(self, depth_u16):
        d = np.ascontiguousarray(depth_u16, dtype=np.uint16)
        return _lib.xs_refshape_process_frame_host(self.h, d.ctypes.data)


def _reference_tsdf(fn, planes, width, depth_dev, rows, cols, intr4, res, voxel_size, R, t, tranc_dist, gt_dev, with_volumes):
    """One of the two reference-signature TSDF launchers: (`planes` sums, and with_volumes `planes` per-voxel volumes, the last one the count); R and t have
    `width` floats per entry."""
    k, r3 = np.ascontiguousarray(intr4, np.float32), np.ascontiguousarray(res, np.int32)
    R, t = np.ascontiguousarray(R, np.float32).reshape(9 * width), np.ascontiguousarray(t, np.float32).reshape(3 * width)
    n = int(r3[0]) * int(r3[1]) * int(r3[2])
    out = np.zeros(planes, np.float32)
    vols = np.zeros(planes * n if with_volumes else 1, np.float32)
    rc = fn(depth_dev.data_ptr(), cols * 2, rows, cols, k.ctypes.data_as(_f32p), r3.ctypes.data_as(_i32p), voxel_size, R.ctypes.data_as(_f32p),
            t.ctypes.data_as(_f32p), tranc_dist, gt_dev.data_ptr(), int(with_volumes), out.ctypes.data_as(_f32p), vols.ctypes.data_as(_f32p) if with_volumes else None)
    assert rc == 0
    if not with_volumes:
        return out
    v = vols.reshape(planes, n)
    return out, (*v[:-1], v[-1].view(np.int32))


def reference_tsdf_hessian(depth_dev, rows, cols, intr4, res, voxel_size, R_dual, t_dual, tranc_dist, gt_dev, with_volumes=False):
    """ComputeLocalTsdf_hessian through its TsdfFusion.h:48-53 signature (xs_launchers.hpp): float4 {loss, gradient, second
    derivative, count} and, with_volumes, the per-voxel (real, grad, hessian, count) volumes."""
    return _reference_tsdf(_lib.xs_refshape_hessian, 4, 4, depth_dev, rows, cols, intr4, res, voxel_size, R_dual, t_dual, tranc_dist, gt_dev, with_volumes)


def reference_tsdf_loss(depth_dev, rows, cols, intr4, res, voxel_size, R9, t3, tranc_dist, gt_dev, with_volumes=False):
    """ComputeLocalTsdf_loss through its TsdfFusion.h:55-60 signature: float2 {loss, count} (+ the (real, count) volumes)."""
    return _reference_tsdf(_lib.xs_refshape_loss, 2, 1, depth_dev, rows, cols, intr4, res, voxel_size, R9, t3, tranc_dist, gt_dev, with_volumes)
