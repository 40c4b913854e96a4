"""CPU-only: the host's side of global relocalisation — pose_candidates, the ranking of
x-slam_amd/host/score_host.hpp under the sanitizers, and the oracle twin of the GPU suite's global-relocalisation case."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import independent_cases as ic
import newton_cases as nc
import score_cases as sc


@pytest.fixture(scope="module")
def pl():
    return importlib.import_module("x-slam_amd.pipeline")


def halton_by_hand(i, base):
    """The radical inverse written digit by digit (exact fractions for the checks below)."""
    digits = []
    while i:
        digits.append(i % base)
        i //= base
    return sum(d / base ** (k + 1) for k, d in enumerate(digits))


def test_pose_candidates(pl):
    """Shape, dtype, determinism; candidates 0, 1, 2 against hand-computed Halton points (i + 1 = 1, 2, 3 in bases 2, 3, 5, 7, 11, 13) and
    the real exponential (nc.twist_matrix); orthonormal rotation blocks; zero imaginary parts."""
    rng = np.random.default_rng(3)
    center = nc.twist_matrix(rng.normal(size=6) * [1.0, 1.0, 1.0, 0.5, 0.5, 0.5])
    c = pl.pose_candidates(center, 0.9, 0.6, 300)
    assert c.shape == (300, 4, 4, 2) and c.dtype == np.float32
    assert pl.pose_candidates(center, 0.9, 0.6, 300).tobytes() == c.tobytes()
    assert pl.pose_candidates(sc.as_c2v32(center), 0.9, 0.6, 300).tobytes() == pl.pose_candidates(center.astype(np.float32), 0.9, 0.6, 300).tobytes()
    assert pl.pose_candidates(center, 0.9, 0.6, 7).tobytes() == c[:7].tobytes()         # candidate i does not depend on n
    assert pl.pose_candidates(center, 0.9, 0.6, 0).shape == (0, 4, 4, 2)
    # halton(1 .. 3, base): 1/2, 1/4, 3/4;  1/3, 2/3, 1/9;  1/5, 2/5, 3/5;  1/7, 2/7, 3/7;  1/11, 2/11, 3/11;  1/13, 2/13, 3/13
    hand = np.array([[1 / 2, 1 / 3, 1 / 5, 1 / 7, 1 / 11, 1 / 13], [1 / 4, 2 / 3, 2 / 5, 2 / 7, 2 / 11, 2 / 13], [3 / 4, 1 / 9, 3 / 5, 3 / 7, 3 / 11, 3 / 13]])
    for i in range(3):
        assert np.allclose([halton_by_hand(i + 1, b) for b in (2, 3, 5, 7, 11, 13)], hand[i], rtol=0, atol=1e-15)
        u = 2.0 * hand[i] - 1.0
        want = center @ nc.twist_matrix(np.concatenate([u[:3] * 0.9, u[3:] * 0.6]))
        assert np.abs(c[i, ..., 0] - want).max() <= 1e-6, (i, np.abs(c[i, ..., 0] - want).max())
    assert np.allclose(c[0, ..., 0], center @ nc.twist_matrix([0, -0.3, -0.54, -0.6 * 5 / 7, -0.6 * 9 / 11, -0.6 * 11 / 13]), rtol=0, atol=1e-6)
    R = c[:, :3, :3, 0].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-6
    assert np.all(c[..., 1] == 0) and np.all(c[:, 3, :, 0] == [0, 0, 0, 1])
    # the twists stay inside the box and fill it: camera-frame translation V v within sqrt(3) box_t, rotation angle within sqrt(3) box_r
    rel = np.linalg.inv(center) @ c[..., 0].astype(np.float64)
    ang = np.arccos(np.clip((np.trace(rel[:, :3, :3], axis1=1, axis2=2) - 1) / 2, -1, 1))
    assert ang.max() <= 0.6 * 3 ** 0.5 + 1e-6 and ang.max() > 0.6 and np.linalg.norm(rel[:, :3, 3], axis=1).max() <= 0.9 * 3 ** 0.5 + 1e-6


def test_score_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/score_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/score_selftest.cpp):
    the stable top-K with ties, K > P, all-zero scores, the winner rule skipping failed loops, nothing ended ok."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "score_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(root, "x-slam_amd", "host"), os.path.join(root, "tests", "cxx", "score_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_ranking_twin_equals_the_rule():
    """score_cases.top_k (what the twin below ranks with) restates score_host.hpp's rule: descending score, ties to the lower index."""
    s = np.array([90.0, 2.0, 90.0, 0.0, 195.0, 90.0])
    assert list(sc.top_k(s, 4)) == [4, 0, 2, 5] and list(sc.top_k(s, 60)) == [4, 0, 2, 5, 1, 3] and list(sc.top_k(np.zeros(5), 3)) == [0, 1, 2]
    assert sc.S(10.0, 100.0) == 90.0


def test_oracle_twin_of_global_relocalisation(oracle, pl):
    """The conditions the GPU suite asserts of KinectFusion.relocalize_global, pinned on the reference alone at 64^3: scene S3 fused at the
    synthetic poses, a start 0.883 m and 50.6 degrees off the last frame's pose, 2048 Halton candidates in a 0.9 m / 0.9 rad box around the
    start, oracle.tsdf_loss per candidate, the best 8 by S = count - sum loss refined by the Gauss-Newton twin for 10 iterations.  Gauss-Newton
    from the start itself fails or ends far off; the global search ends within 1 cm and 0.5 degrees of the truth with S >= 0.98 x the
    truth's own."""
    n = 64
    prm, gt, ds, truth = nc.s3_map_and_truth(oracle, n)
    args = (oracle, ds, [n, n, n], prm["tsdf_voxel_size"], ic.tranc_dist(prm), ic.intr_of(prm), gt)
    start = sc.global_start(truth)
    dt, dr = sc.pose_error(start, truth)
    print(f"start: {dt:.3f} m, {dr:.1f} degrees off")
    assert 0.85 < dt < 0.92 and 50.0 < dr < 51.0
    (s_truth,), (c_truth,) = sc.oracle_scores(*args, [truth])
    (s_start,), (c_start,) = sc.oracle_scores(*args, [start])
    S_truth = float(sc.S(s_truth, c_truth))
    print("S at truth", S_truth, "count", c_truth, " S at start", float(sc.S(s_start, c_start)))
    ok0, end0 = sc.gn_twin_loop(*args, start, sc.GLOBAL_ITERATIONS, sc.GLOBAL_DAMPING)
    far0 = sc.pose_error(end0.real, truth)
    print("Gauss-Newton from the start: ok", ok0, "ends", far0)
    assert not ok0 or far0[0] > 0.10
    cands = pl.pose_candidates(start, sc.GLOBAL_BOX_T, sc.GLOBAL_BOX_R, sc.GLOBAL_CANDIDATES)[..., 0].astype(np.float64)
    ok, winner, rep = sc.global_twin(*args, cands, sc.GLOBAL_KEEP, sc.GLOBAL_ITERATIONS, sc.GLOBAL_DAMPING)
    assert ok
    err = sc.pose_error(winner, truth)
    print("winner", rep["index"], "S before", rep["S_before"], "after", rep["S_after"], "of", S_truth, "error", err, "ok", rep["refined_ok"])
    assert err[0] <= 0.01 and err[1] <= 0.5
    assert rep["S_after"] >= 0.98 * S_truth and rep["S_after"] > rep["S_before"]
