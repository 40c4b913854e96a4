"""Scoring many pose hypotheses in one band pass and global relocalisation: what the CPU and GPU suites share —
the pose sets of the kernel-level tests, the derived tolerance, the start and candidates of the global-relocalisation case and its numpy /
oracle twin (oracle.tsdf_loss per hypothesis, the Gauss-Newton twin of tests/newton_cases.py around the oracle's six-pose kernel).
Extends tests/newton_cases.py.  Test infrastructure."""
import numpy as np

import newton_cases as nc

# |band - dense| <= SUM_BOUND * dense.  Derived, not measured: both sides add the same float32 terms, all >= 0; the dense kernel adds them in
# double; the band kernel adds each 64-entry chunk in a six-level pairwise float tree (relative error <= 6 * 2^-24 to first order, rounded up
# to 8 for the higher-order terms and the double additions after it) and everything after that in double.
SUM_BOUND = 8.0 * 2.0 ** -24

GLOBAL_START_TWIST = 2.5 * np.array([0.25, -0.2, 0.15, 0.2, -0.25, 0.15])   # 0.883 m and 50.6 degrees off
GLOBAL_BOX_T, GLOBAL_BOX_R, GLOBAL_CANDIDATES, GLOBAL_KEEP, GLOBAL_ITERATIONS, GLOBAL_DAMPING = 0.9, 0.9, 2048, 8, 10, 1e-3


def v2c_f32(c2v_real):
    """(Rv2c [3, 3], tv2c [3]) float32 of a real camera2volume: nc.v2c_of's rounding."""
    v = nc.v2c_of(c2v_real)
    return v[:3, :3].astype(np.float32), v[:3, 3].astype(np.float32)


def kernel_poses(truth_c2v, count=200, seed=11):
    """The camera2volume poses [count, 4, 4] (float64) of the kernel-level tests: the truth; 150 camera-frame perturbations of it by twists
    of norm 0.01 .. 0.8 (m / rad, log-uniform: from all of the frame in view to a fraction of it); the camera turned by 180 degrees about its
    y axis (inv_z < 0 everywhere: count 0); one 20 m away (count 0); the rest random rigid poses."""
    rng = np.random.default_rng(seed)
    truth = np.asarray(truth_c2v, np.float64)
    out = [truth]
    for _ in range(150):
        d = rng.normal(size=6)
        out.append(truth @ nc.twist_matrix(d / np.linalg.norm(d) * np.exp(rng.uniform(np.log(0.01), np.log(0.8)))))
    out.append(truth @ nc.twist_matrix(np.array([0, 0, 0, 0, np.pi, 0.0])))
    far = truth.copy(); far[:3, 3] += [20.0, 0.0, 0.0]
    out.append(far)
    while len(out) < count:
        out.append(nc.twist_matrix(rng.normal(size=6) * np.array([1.5, 1.5, 1.5, 0.6, 0.6, 0.6])) @ truth)
    return np.stack(out[:count])
TURNED, FAR = 151, 152   # their indices in kernel_poses


def as_c2v32(c2v_real):
    """[..., 4, 4] real -> [..., 4, 4, 2] float32 with zero imaginary parts."""
    m = np.zeros(np.shape(c2v_real) + (2,), np.float32)
    m[..., 0] = c2v_real
    return m


def S(sum_loss, count):
    """The truncated-quadratic inlier score: a kept voxel counts 1 - r^2, a dropped one 0."""
    return np.asarray(count, np.float64) - np.asarray(sum_loss, np.float64)


def top_k(scores, K):
    """Indices of the min(K, P) highest scores, best first, ties to the lower index."""
    return np.argsort(-np.asarray(scores, np.float64), kind="stable")[:K]


def pose_error(c2v_real, truth_real):
    """(translation distance in metres, rotation angle in degrees) between two real camera2volume poses."""
    a, b = np.asarray(c2v_real, np.float64), np.asarray(truth_real, np.float64)
    c = (np.trace(a[:3, :3].T @ b[:3, :3]) - 1.0) / 2.0
    return float(np.linalg.norm(a[:3, 3] - b[:3, 3])), float(np.degrees(np.arccos(np.clip(c, -1.0, 1.0))))


def global_start(truth_real):
    return np.asarray(truth_real, np.float64) @ nc.twist_matrix(GLOBAL_START_TWIST)


def oracle_scores(oracle, depth_m, res, vs, trunc, k4, gt, c2vs_real):
    """(sum loss [P], count [P]) of oracle.tsdf_loss at the float32 inverse of every camera2volume."""
    out = np.zeros((len(c2vs_real), 2))
    for p, m in enumerate(c2vs_real):
        R, t = v2c_f32(m)
        out[p] = oracle.tsdf_loss(depth_m, res, vs, R, t, trunc, k4, gt)
    return out[:, 0], out[:, 1]


def gn_twin_loop(oracle, depth_m, res, vs, trunc, k4, gt, c2v0_real, iters, damping):
    """The numpy twin of one frame of RelocalizeGaussNewtonBatch without a loss pass: per iteration the oracle's six-pose sums
    (nc.gn_twin_sums), then gn_loop_step — fewer than six voxels or a damped system that is not positive definite end the loop not ok.
    Returns (ok, camera2volume complex64)."""
    damping = float(np.float32(damping))
    c2v = np.asarray(c2v0_real, np.float32).astype(np.complex64)
    for _ in range(iters):
        s = nc.gn_twin_sums(oracle, depth_m, res, vs, trunc, k4, gt, c2v)
        if s[28] < 6:
            return False, c2v
        x = nc.damped_solve(s, damping)
        if x is None:
            return False, c2v
        c2v = nc.apply_step(x, c2v)
    return True, c2v


def global_twin(oracle, depth_m, res, vs, trunc, k4, gt, candidates_real, keep, iters, damping):
    """RelocalizeGlobal restated: score, keep the top `keep`, refine each with gn_twin_loop, score again, the best S among the ok ones.
    Returns (ok, winner c2v real [4, 4] or None, report dict as KinectFusion.relocalize_global's)."""
    args = (oracle, depth_m, res, vs, trunc, k4, gt)
    s0, c0 = oracle_scores(*args, candidates_real)
    top = top_k(S(s0, c0), keep)
    loops = [gn_twin_loop(*args, candidates_real[i], iters, damping) for i in top]
    refined = [c.real.astype(np.float64) for _, c in loops]
    s1, c1 = oracle_scores(*args, refined)
    S1 = S(s1, c1)
    oks = np.array([ok for ok, _ in loops])
    report = dict(index=-1, S_before=0.0, S_after=0.0, sum_loss_after=0.0, count_after=0.0, refined_ok=int(oks.sum()), refined=refined, oks=oks)
    if not oks.any():
        return False, None, report
    w = int(top_k(np.where(oks, S1, -np.inf), 1)[0])
    report.update(index=int(top[w]), S_before=float(S(s0, c0)[top[w]]), S_after=float(S1[w]), sum_loss_after=float(s1[w]), count_after=float(c1[w]))
    return True, refined[w], report
