"""CPU-only: the host's side of the exact-Hessian (Newton) relocalisation (x-slam_amd/host/newton_host.hpp through xs_host_newton_seeded_poses /
xs_host_newton_step) and the oracle twin of the loop the GPU suite compares RelocalizeNewtonBatch with (tests/newton_cases.py)."""
import importlib

import numpy as np
import pytest

import independent_cases as ic
import newton_cases as nc
from conftest import ulp_diff


@pytest.fixture(scope="module")
def pl():
    return importlib.import_module("x-slam_amd.pipeline")


def random_rigid(rng):
    """A camera2volume [4, 4, 2] float32 with a zero imaginary part: a random rotation of up to a radian and a translation of metres."""
    xi = rng.normal(size=6) * np.array([1.5, 1.5, 1.5, 0.6, 0.6, 0.6])
    c2v = np.zeros((4, 4, 2), np.float32)
    c2v[..., 0] = nc.twist_matrix(xi)
    return c2v


def test_seeded_poses_equal_pair_pose_bit_for_bit(pl):
    """xs_host_newton_seeded_poses: the 21 real parts are the same bits, and with that real part as v2c every pair is
    independent_cases.pair_pose(v2c, a, b, cross=True) — both round the same float64 products once (ulp distance 0: the sign of a zero that
    stands for an absent entry is not compared)."""
    rng = np.random.default_rng(20261017)
    for trial in range(50):
        c2v = random_rigid(rng)
        R, t = pl.host_newton_seeded_poses(c2v)
        assert R.shape == (21, 3, 3, 4) and t.shape == (21, 3, 4)
        for p in range(1, 21):
            assert np.array_equal(R[p, ..., 0].view(np.uint32), R[0, ..., 0].view(np.uint32)), (trial, p)
            assert np.array_equal(t[p, :, 0].view(np.uint32), t[0, :, 0].view(np.uint32)), (trial, p)
        v2c = np.eye(4)
        v2c[:3, :3], v2c[:3, 3] = R[0, ..., 0], t[0, :, 0]
        # the real part is the inverse of c2v to float rounding
        assert np.abs(v2c @ c2v[..., 0].astype(np.float64) - np.eye(4)).max() < 2e-6, trial
        wantR, wantt = nc.pair_poses(v2c)
        assert ulp_diff(R, wantR).max() == 0 and ulp_diff(t, wantt).max() == 0, trial
        # and the seeds are there: every pair has both first-order parts, every pair that has one a second-order part
        assert all(np.abs(R[p, ..., 1]).max() + np.abs(t[p, :, 1]).max() > 0 for p in range(21))
        assert np.abs(R[nc.PAIRS.index((3, 4)), ..., 3]).max() > 0 and np.abs(t[nc.PAIRS.index((0, 4)), :, 3]).max() > 0
        assert not R[nc.PAIRS.index((0, 1)), ..., 3].any() and not t[nc.PAIRS.index((0, 1)), :, 3].any()   # two translations commute


def random_sums(rng, definite=True):
    B = rng.normal(size=(6, 6))
    H = B @ B.T * 1e3 + np.eye(6) * 10.0
    if not definite:
        w, V = np.linalg.eigh(H)
        w[0] = -w[-1]   # (no damping of up to diag H makes this positive definite)
        H = V @ np.diag(w) @ V.T
    s = np.zeros(29)
    s[:21] = H[np.triu_indices(6)]
    s[21:27] = rng.normal(size=6) * 5.0
    s[27], s[28] = 12.5, 4000.0
    return s


def test_newton_step_against_a_numpy_twin(pl):
    """xs_host_newton_step against Cholesky in double on (H + damping diag H) and se3_exp_c64 (the reference's se3Exp restated in
    tests/test_gauss_newton_gpu.py): pose entries within 1e-6, the bound of that file's twin test for the same host algebra.  An indefinite
    H and count < 6: -1, pose untouched."""
    rng = np.random.default_rng(7)
    for trial in range(40):
        c2v = random_rigid(rng)
        s = random_sums(rng)
        damping = float(np.float32(rng.choice([0.0, 1e-3, 0.1])))
        taken, got = pl.host_newton_step(s, damping, c2v)
        assert taken
        x = nc.damped_solve(s, damping)
        assert x is not None and np.abs(x).max() < 1.0
        want = nc.apply_step(x, c2v[..., 0].astype(np.complex64))
        assert np.abs(got[..., 0] - want.real).max() <= 1e-6, (trial, np.abs(got[..., 0] - want.real).max())
        assert np.all(got[..., 1] == 0)
        # refusals leave the pose as it was
        for bad in (random_sums(rng, definite=False), np.concatenate([s[:28], [5.0]])):
            assert bad[28] < 6 or nc.damped_solve(bad, damping) is None
            taken, same = pl.host_newton_step(bad, damping, c2v)
            assert not taken and np.array_equal(same.view(np.uint32), c2v.view(np.uint32)), trial
    # a Hessian that only the damping makes definite is accepted with it and refused without
    s = random_sums(rng)
    H = nc.sym6(s[:21]); w, V = np.linalg.eigh(H); w[0] = -1e-6 * w[-1]
    s[:21] = (V @ np.diag(w) @ V.T)[np.triu_indices(6)]
    assert not pl.host_newton_step(s, 0.0, random_rigid(rng))[0]
    assert (nc.damped_solve(s, 0.5) is not None) == pl.host_newton_step(s, 0.5, random_rigid(rng))[0]


def test_newton_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/newton_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run
    (tests/cxx/newton_selftest.cpp), as tests/test_abi_cpu.py does for the rest of the header-only host code."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "newton_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(root, "x-slam_amd", "host"), os.path.join(root, "tests", "cxx", "newton_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


INDEFINITE_START = np.array([-0.09969, 0.01168, -0.08474, -0.03559, 0.00334, -0.0022])   # tests/test_newton_gpu.py: the fallback's start


@pytest.mark.parametrize("n", [64, 128])
def test_oracle_newton_twin_converges(oracle, n):
    """The loop the GPU test is compared with, pinned on the CPU: oracle.tsdf_hessian called 21 times with the pair_pose seeds gives H and g
    on scene S3, and the numpy Newton loop around it (newton_cases.newton_twin_loop) converges from the Gauss-Newton twin test's start: final
    loss < 0.5 x initial, monotonically, no fallback, one count for all 21 pairs, and its gradient is the six-pose kernel's 2 J^T r.  The
    same twin from INDEFINITE_START meets an indefinite Hessian on its first iteration and takes the Gauss-Newton step — the conditions the GPU suite asserts of the product (checked at its size, 128^3, too)."""
    prm, gt, ds, t_true = nc.s3_map_and_truth(oracle, n)
    args = (oracle, ds, [n, n, n], prm["tsdf_voxel_size"], ic.tranc_dist(prm), ic.intr_of(prm), gt)
    start = nc.twist_matrix(nc.START_TWIST) @ t_true
    hist, poses, fell, sums = nc.newton_twin_loop(*args, start, 5, 1e-3)
    assert hist[-1] < 0.5 * hist[0] and np.all(np.diff(hist) <= 1e-9), hist
    assert not fell.any() and sums[:, 28].min() > 1000
    assert np.all(poses.imag == 0)
    gn = nc.gn_twin_sums(*args, poses[-1])
    JtJ = nc.sym6(gn[:21])
    # the gradient is the same derivative in both kernels: dL / dtheta = 2 J^T r (assert_identity's scale and bound)
    diag = np.diag(JtJ)
    assert np.all(np.abs(sums[-1][21:27] - 2 * gn[21:27]) <= 1e-4 * 2 * np.sqrt(diag * gn[27]))
    # the fallback: an indefinite H at the first iteration, the Gauss-Newton step taken, the loop goes on
    hist, poses, fell, sums = nc.newton_twin_loop(*args, nc.twist_matrix(INDEFINITE_START) @ t_true, 2, 1e-3)
    if n == 128:
        assert fell[0] and np.linalg.eigvalsh(nc.sym6(sums[0][:21])).min() < 0, (fell, sums[0][:21])
        assert sums[:, 28].min() > 1000 and hist[1] < hist[0]
