"""CPU-only: the host's side of view scoring — the float32 model of xs_score_views' contract against its plain-Python
restatement and against the known answers, the selection rule of x-slam_amd/host/view_host.hpp under the sanitizers, the grid's size and
the bindings."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import view_cases as vc


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module("x-slam_amd.capi")


def test_model_equals_its_restatement():
    """The vectorised numpy model against the triple loop on res (6, 5, 7), a 5 x 3 lattice and four poses: a camera in front of the volume,
    one inside it, one turned away, one random.  Random states, so unknown, free, hits and frontier crossings all occur."""
    rng = np.random.default_rng(4)
    X, Y, Z = 6, 5, 7
    states = rng.integers(0, 3, size=(Z, Y, X)).astype(np.uint8)
    states[:3] = np.where(states[:3] == vc.OCCUPIED, vc.FREE, states[:3])      # (a surface right at the front would end every ray at once)
    vs = vc.f32(0.1)
    eye = np.eye(3, dtype=vc.f32)
    R = [eye, vc.rot_y(0.4), vc.rot_y(np.pi), vc.random_rotation(rng)]
    t = [np.array([0.3, 0.25, -0.3], vc.f32), np.array([0.3, 0.25, 0.05], vc.f32), np.array([0.3, 0.25, -0.3], vc.f32), np.array([0.2, 0.3, 0.3], vc.f32)]
    kw = dict(rays=(5, 3), t_near=0.2, t_far=1.3, step=0.07)
    total = np.zeros(4, np.uint64)
    for p in range(4):
        got = vc.model(states, R[p], t[p], (60.0, 55.0, 31.5, 23.5), 48, 64, vs, **kw)
        want = vc.restatement(states, R[p], t[p], (60.0, 55.0, 31.5, 23.5), 48, 64, vs, **kw)
        print(p, got, want)
        assert got.dtype == np.uint32 and np.array_equal(got, want), p
        total += got
    assert np.all(total > 0) and not vc.model(states, R[2], t[2], (60.0, 55.0, 31.5, 23.5), 48, 64, vs, **kw).any()


def test_known_answers():
    """The table of DESIGN.md section 4.18: a 64^3 volume, half of it never observed, a floor of occupied voxels under free space, five
    cameras turned about y.  103 samples per ray; with min_hits 1200 the next best view is a = 0.5 — a = 1.0 sees more unknown space but no
    surface."""
    states = vc.known_states()
    assert len(vc.sample_depths(0.2, 5.0, vc.KNOWN_VOXEL)) == 103
    R, t = vc.known_poses()
    got = vc.model_poses(states, R, t, vc.INTR, vc.ROWS, vc.COLS, vc.KNOWN_VOXEL)
    print(got)
    assert np.array_equal(got, vc.KNOWN_COUNTS)
    assert vc.next_best_view(got, vc.KNOWN_MIN_HITS) == vc.KNOWN_BEST == 2
    assert got[3, 0] > got[2, 0] and got[3, 2] == 0 and vc.next_best_view(got, 0) == 3
    # the volumes the states stand for give the states back, at both weight gates
    value, weight = vc.volumes_of(states)
    assert np.array_equal(vc.states_of(value, weight), states) and not vc.states_of(value, weight, 2).any()
    assert np.array_equal(vc.states_of(value, weight, 0), states)               # below 1 means 1
    assert vc.states_of(np.float32(-0.0), 1) == vc.FREE and vc.states_of(np.float32(-1e-30), 1) == vc.OCCUPIED


def test_view_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/view_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/view_selftest.cpp):
    ties, nobody qualifies, P = 1, min_hits = 0.  The Python twin the GPU suite picks with restates the same rule."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "view_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(root, "x-slam_amd", "host"), os.path.join(root, "tests", "cxx", "view_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    a = np.array([[100, 5, 10, 1], [900, 0, 0, 7], [300, 9, 10, 2], [300, 1, 50, 3], [50, 2, 400, 0], [300, 4, 9, 4]], np.uint32)
    assert [vc.next_best_view(a, h) for h in (10, 11, 51, 401, 0, 9)] == [2, 3, 4, -1, 1, 2]
    assert vc.next_best_view(a[:0], 0) == -1 and vc.next_best_view(a[5:], 9) == 0 and vc.next_best_view(a[5:], 10) == -1


def test_view_grid_bytes(capi):
    """Positive and monotone for valid resolutions, 0 for a non-positive one, and at least a 16-byte word per brick of 4 x 4 x 4 voxels
    (partial bricks included)."""
    bricks = lambda r: -(-r[0] // 4) * -(-r[1] // 4) * -(-r[2] // 4)
    sizes = [(1, 1, 1), (4, 4, 4), (5, 4, 4), (8, 8, 8), (20, 18, 13), (64, 64, 64), (65, 64, 64), (512, 512, 512), (1024, 1024, 1024)]
    got = [capi.view_grid_bytes(r) for r in sizes]
    print(dict(zip(sizes, got)))
    for r, b in zip(sizes, got):
        assert b >= bricks(r) * 16 > 0 and b % 16 == 0, r
    assert got == sorted(got) and got[1] < got[2] and got[5] < got[6]
    assert got[7] < 40 << 20                                                     # 32 MiB of bricks at 512^3, where the two volumes take 1 GiB
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (-8, -8, -8)):
        assert capi.view_grid_bytes(bad) == 0, bad


def test_bindings_exist(capi):
    """The entry points of every layer: the library's symbols with their ctypes signatures, the options struct's size, the orchestrator's
    C ABI and the methods of KinectFusion (ShardedKinectFusion inherits them; in shard mode they raise XsError — the GPU suite)."""
    pl = importlib.import_module("x-slam_amd.pipeline")
    sh = importlib.import_module("x-slam_amd.sharded")
    for n in ("xs_view_grid_bytes", "xs_view_grid_build", "xs_view_grid_expand", "xs_score_views"):
        assert n in capi._SIGS and hasattr(capi._lib, n), n
    for n in ("xs_kf_score_views", "xs_kf_next_best_view"):
        assert n in pl._SIGS and hasattr(pl._lib, n), n
    o = capi.view_opts()
    assert o.struct_bytes == 24 and (o.rays_x, o.rays_y, o.t_near, o.t_far, o.step) == (0, 0, 0.0, 0.0, 0.0)
    o = capi.view_opts((9, 7), 0.2, 2.0, 0.05)
    assert (o.rays_x, o.rays_y) == (9, 7) and o.t_far == 2.0 and o.step == np.float32(0.05)
    assert capi.VIEW_MAX_POSES == 4096 and capi.abi_version() == 3
    for cls in (pl.KinectFusion, sh.ShardedKinectFusion):
        assert callable(cls.score_views) and callable(cls.next_best_view)
