"""The exact pose Hessian and the Newton relocalisation loop: what the CPU and GPU suites share — the 21 seeded
dual-complex poses through independent_cases.pair_pose, the oracle's 29 sums from 21 calls of its Hessian kernel, and the numpy twin of the
host loop.  Extends tests/independent_cases.py.  Test infrastructure."""
import numpy as np

import independent_cases as ic
from test_gauss_newton_gpu import se3_exp_c64, twist_matrix   # noqa: F401  (the reference's se3Exp restated in complex64; the start twist's exponential)

PAIRS = [(a, b) for a in range(6) for b in range(a, 6)]
DIAG = [PAIRS.index((a, a)) for a in range(6)]
H2 = ic.H2
START_TWIST = np.array([0.008, -0.006, 0.005, 0.004, -0.005, 0.006])   # the Gauss-Newton twin test's start


def pair_poses(v2c):
    """The 21 dual-complex poses of a pass at the real pose v2c (4 x 4 float64 holding float32 values): R [21, 3, 3, 4], t [21, 3, 4]."""
    Rt = [ic.pair_pose(v2c, a, b, cross=True) for a, b in PAIRS]
    return np.stack([r for r, _ in Rt]), np.stack([t for _, t in Rt])


def v2c_of(c2v_real):
    """The real volume-to-camera pose of a camera2volume, inverted in double and rounded to float32 (held in float64)."""
    return np.linalg.inv(np.asarray(c2v_real, np.float64)).astype(np.float32).astype(np.float64)


def sums_from_launches(outs):
    """The 29 raw sums of the one-launch kernel from the 21 per-pair {loss, grad, hessian, count} of the single-pair kernel."""
    outs = np.asarray(outs, np.float64)
    assert outs.shape == (21, 4)
    return np.concatenate([outs[:, 2], outs[DIAG, 1], outs[:1, 0], outs[:1, 3]])


def oracle_pose_hessian(oracle, depth_m, res, vs, trunc, k4, gt, v2c):
    """29 raw sums at the real pose v2c from 21 calls of the oracle's dual-complex kernel; the 21 counts (equal when every evaluation
    keeps the same voxels)."""
    R, t = pair_poses(v2c)
    outs = []
    for p in range(21):
        o = oracle.tsdf_hessian(depth_m, res, vs, R[p], t[p], trunc, k4, gt)
        outs.append(o[0] if isinstance(o, tuple) else o)
    outs = np.asarray(outs, np.float64)
    return sums_from_launches(outs), outs[:, 3]


def scale(raw):
    s = np.array(raw, np.float64)
    s[:21] /= H2 * H2
    s[21:27] /= H2
    return s


def sym6(upper21):
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = upper21
    return A + np.triu(A, 1).T


def damped_solve(s, damping):
    """x of (A + damping diag A) x = -b by Cholesky in double, A = s[:21], b = s[21:27]; None where it is not positive definite."""
    A = sym6(s[:21])
    A[np.diag_indices(6)] *= 1.0 + float(damping)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, -np.asarray(s[21:27], np.float64)))


def apply_step(x, c2v_c64):
    return (se3_exp_c64(x.astype(np.float32).astype(np.complex64)) @ c2v_c64).astype(np.complex64)


def gn_twin_sums(oracle, depth_m, res, vs, trunc, k4, gt, c2v_c64):
    """The Gauss-Newton twin's scaled sums (tests/test_gauss_newton_gpu.py: poses inverse(se3Exp(i h e_k) c2v) in complex64)."""
    h = np.float32(1e-7)
    Rs = np.zeros((6, 3, 3, 2), np.float32); ts = np.zeros((6, 3, 2), np.float32)
    for k in range(6):
        xi = np.zeros(6, np.complex64); xi[k] = 1j * h
        v2c = np.linalg.inv((se3_exp_c64(xi) @ c2v_c64).astype(np.complex128)).astype(np.complex64)
        Rs[k, ..., 0], Rs[k, ..., 1] = v2c[:3, :3].real, v2c[:3, :3].imag
        ts[k, :, 0], ts[k, :, 1] = v2c[:3, 3].real, v2c[:3, 3].imag
    s = oracle.tsdf_gn_terms(depth_m, res, vs, Rs, ts, trunc, k4, gt).copy()
    s[:21] /= float(h) ** 2
    s[21:27] /= float(h)
    return s


def newton_twin_loop(oracle, depth_m, res, vs, trunc, k4, gt, c2v0_real, iters, damping):
    """The numpy twin of RelocalizeNewtonBatch for one frame: per iteration the oracle's 29 sums at v2c_of(c2v), the loss, the damped solve in
    double, the update se3Exp(x) c2v in complex64; where the damped Hessian is not positive definite, the Gauss-Newton twin's step for that
    iteration.  Returns (losses [iters + 1], poses after each iteration [iters, 4, 4] complex64, fallback flags [iters], scaled sums [iters + 1, 29])."""
    damping = float(np.float32(damping))
    c2v = np.asarray(c2v0_real, np.float32).astype(np.complex64)
    hist, poses, fell, sums = [], [], [], []
    for it in range(iters + 1):
        raw, counts = oracle_pose_hessian(oracle, depth_m, res, vs, trunc, k4, gt, v2c_of(c2v.real))
        assert np.all(counts == counts[0]), counts
        s = scale(raw)
        sums.append(s)
        hist.append(s[27] / s[28])
        if it == iters:
            break
        x = damped_solve(s, damping)
        fell.append(x is None)
        if x is None:
            x = damped_solve(gn_twin_sums(oracle, depth_m, res, vs, trunc, k4, gt, c2v), damping)
            assert x is not None
        c2v = apply_step(x, c2v)
        poses.append(c2v.copy())
    return np.array(hist), np.array(poses), np.array(fell), np.array(sums)


def s3_map_and_truth(oracle, n, frames=6):
    """CPU: the S3 map of the first `frames` frames at their synthetic poses through the oracle's integrate, the last frame's scaled depth
    and its camera2volume."""
    prm = ic.synth.s1_params(n)
    res = [n, n, n]
    v, w, g = oracle.new_volume(res)
    for k in range(frames):
        T = ic.s1_transforms(k, prm)
        oracle.integrate(oracle.scale_depth(ic.synth.s3_frame(k)), v, w, g, res, ic.tranc_dist(prm), 100, T["Rv2c"], T["tv2c"], ic.intr_of(prm),
                         prm["tsdf_voxel_size"])
    T = ic.s1_transforms(frames - 1, prm)
    v2c = np.eye(4); v2c[:3, :3] = np.asarray(T["Rv2c"])[..., 0]; v2c[:3, 3] = np.asarray(T["tv2c"])[..., 0]
    return prm, v, oracle.scale_depth(ic.synth.s3_frame(frames - 1)), np.linalg.inv(v2c)
