"""ctypes binding of the host orchestrator's C ABI (include/xslam_amd_pipeline.h,
libxslam_host.so built from x-slam_amd/host/).  The orchestrator itself is C++
(KinectFusionReconstruction, mirroring the reference class); this module only lets Python
callers — bench.py and the parity tests — drive it.  No CPU fallback: a missing library is an
ImportError.  This is the import point: every public name of the pipeline_*.py modules beside it, and the
private ones callers use, resolve from here."""
from .pipeline_abi import *  # noqa: F401,F403
from .pipeline_abi import _SIGS, _f32p, _f64p, _i32p, _lib, _sz, _vp  # noqa: F401
from .pipeline_hostmath import *  # noqa: F401,F403
from .pipeline_hostmath import _halton, _real44, _se3_exp  # noqa: F401
from .pipeline_maps import Maps as _Maps
from .pipeline_planning import Planning as _Planning
from .pipeline_reference import ReferenceCallShape, reference_tsdf_hessian, reference_tsdf_loss  # noqa: F401
from .pipeline_tracking import Tracking as _Tracking


class KinectFusion(_Tracking, _Planning, _Maps):
    """Handle to a C++ KinectFusionReconstruction."""

    def __init__(self, params, gt_poses=None):
        self._open(params, "xs_kf_create failed (missing config key, or a retired one set?)")
        if gt_poses is not None:
            g = np.ascontiguousarray(gt_poses, dtype=np.float32).reshape(-1, 32)
            _lib.xs_kf_set_gt_poses(self.h, g.shape[0], g.ctypes.data_as(_f32p))
