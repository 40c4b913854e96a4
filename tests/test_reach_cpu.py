"""CPU-only: the host's side of clearance and reachability — the scipy model the kernels are held to against a
scalar brute force, the snap rule's tie-break, the radius derivation, the selection rule of x-slam_amd/host/view_host.hpp under the
sanitizers, the buffer sizes and the bindings."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import reach_cases as rc
import view_cases as vc


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module("x-slam_amd.capi")


@pytest.mark.parametrize("res", [(7, 6, 5), (5, 4, 9)])
@pytest.mark.parametrize("unknown_blocks", [0, 1])
def test_model_equals_brute_force(res, unknown_blocks):
    """scipy's EDT and label against all-pairs distances and a breadth-first search, R in {1, 3, 9}: R = 9 is longer than every axis, so
    with unknown_blocks the positions outside the volume decide and without it the cap is never reached inside; the states are random
    with few obstacles, so distances above 1 occur."""
    states = rc.random_states(res, seed=3 + res[0], p=(0.08, 0.84, 0.08))
    assert len(np.unique(states)) == 3
    for R in (1, 3, 9):
        got, want = rc.clearance(states, R, unknown_blocks), rc.brute_clearance(states, R, unknown_blocks)
        print(res, unknown_blocks, R, "values", np.unique(want))
        assert got.dtype == np.uint16 and np.array_equal(got, want), (R, np.argwhere(got != want)[:5])
        assert want.max() > 1 or R == 1
        for r2 in sorted({1, 2, R * R}):
            rng = np.random.default_rng(R + r2)
            seeds = np.stack([rng.integers(-1, res[0] + 1, 5), rng.integers(-1, res[1] + 1, 5), rng.integers(-1, res[2] + 1, 5)], axis=1)
            a, b = rc.reached(states, want, r2, seeds), rc.brute_reached(states, want, r2, seeds)
            assert np.array_equal(a, b), (R, r2)
    # no obstacle at all: R^2 everywhere without unknown_blocks, the distance to the outside with it
    free = np.full(states.shape, rc.FREE, np.uint8)
    assert np.array_equal(rc.clearance(free, 3, unknown_blocks), rc.brute_clearance(free, 3, unknown_blocks))
    assert unknown_blocks or np.all(rc.clearance(free, 3, 0) == 9)
    assert not unknown_blocks or rc.clearance(free, 3, 1)[0, 0, 0] == 1


def test_snap_tie_rule():
    """A point whose voxel is not in the mask answers for the nearest mask voxel in the snap cube, ties to the lowest linear index; the
    cube is |v - s|_inf <= snap, so a nearer voxel outside it does not count and a farther one inside it does."""
    X, Y, Z = 9, 8, 7
    field = (np.arange(X * Y * Z) % 50000).astype(np.uint16).reshape(Z, Y, X)
    mask = np.zeros((Z, Y, X), bool)
    vs = 0.1
    p = (np.array([[4, 4, 3]], np.float32) + 0.5) * np.float32(vs)
    r, c, v = rc.query(p, vs, mask, field, snap=3)
    assert (r[0], c[0]) == (0, field[3, 4, 4]) and tuple(v[0]) == (-1, -1, -1)
    for x, y, z in ((5, 4, 3), (4, 5, 3), (4, 4, 4), (3, 4, 3), (4, 3, 3), (4, 4, 2)):   # six voxels at distance 1
        mask[z, y, x] = True
    r, c, v = rc.query(p, vs, mask, field, snap=3)
    assert r[0] == 1 and tuple(v[0]) == (4, 4, 2) and c[0] == field[2, 4, 4]      # the lowest (z Y + y) X + x
    mask[2, 4, 4] = False
    assert tuple(rc.query(p, vs, mask, field, snap=1)[2][0]) == (4, 3, 3)
    mask[3, 3, 4] = False
    assert tuple(rc.query(p, vs, mask, field, snap=1)[2][0]) == (3, 4, 3)
    assert rc.query(p, vs, mask, field, snap=0)[0][0] == 0
    mask[:] = False
    mask[3, 4, 7] = True                                                         # distance 3 along x ...
    mask[5, 6, 6] = True                                                         # ... and (2, 2, 2): 12, inside the cube of snap 2
    assert tuple(rc.query(p, vs, mask, field, snap=3)[2][0]) == (7, 4, 3)
    assert tuple(rc.query(p, vs, mask, field, snap=2)[2][0]) == (6, 6, 5)
    assert rc.query(p, vs, mask, field, snap=1)[0][0] == 0
    mask[3, 4, 4] = True                                                         # its own voxel: no snapping
    r, c, v = rc.query(p, vs, mask, field, snap=3)
    assert (r[0], c[0]) == (1, field[3, 4, 4]) and tuple(v[0]) == (4, 4, 3)
    out = np.array([[-0.01, 0.45, 0.35], [0.45, 0.45, 0.7], [20.0, 0.4, 0.3], [np.nan, 0.4, 0.3]], np.float32)
    r, c, v = rc.query(out, vs, np.ones((Z, Y, X), bool), field, snap=3)
    assert not r.any() and not c.any() and np.all(v == -1)                       # outside the volume: (0, 0), never snapped


def test_radius_derivation():
    """rv = radius / voxel in float32, r2 = max(1, ceil(rv^2)), R the least integer with R^2 >= r2: on and beside integer multiples."""
    assert rc.radius_of(0.0, 0.05) == (1, 1) and rc.radius_of(0.05, 0.05) == (1, 1) and rc.radius_of(0.1, 0.05) == (4, 2)
    assert rc.radius_of(0.5, 0.25) == (4, 2) and rc.radius_of(np.nextafter(np.float32(0.5), np.float32(1)), 0.25) == (5, 3)
    assert rc.radius_of(np.nextafter(np.float32(0.5), np.float32(0)), 0.25) == (4, 2)
    assert rc.radius_of(0.75, 0.25) == (9, 3) and rc.radius_of(0.8, 0.25) == (11, 4) and rc.radius_of(63.75, 0.25) == (65025, 255)
    for k in range(1, 256):
        assert rc.radius_of(0.125 * k, 0.125) == (k * k, k)
    r2, R = rc.radius_of(0.12, 3.0 / 64.0)                                       # 2.56 voxels: 6.5536 -> 7
    assert (r2, R) == (7, 3)


def test_reach_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/view_host.hpp's next_reachable_view and reach_radius compiled with -fsanitize=address,undefined
    -fno-sanitize-recover and run (tests/cxx/reach_selftest.cpp).  The Python twins the GPU suite uses restate the same rules."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "reach_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(root, "x-slam_amd", "host"), os.path.join(root, "tests", "cxx", "reach_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    a = np.array([[100, 5, 10, 1], [900, 0, 0, 7], [300, 9, 10, 2], [300, 1, 50, 3], [50, 2, 400, 0], [300, 4, 9, 4]], np.uint32)
    r1 = [1, 0, 0, 1, 1, 1]
    assert [rc.next_reachable_view(a, r1, h) for h in (10, 9, 0, 51, 401)] == [3, 3, 3, 4, -1]
    assert [rc.next_reachable_view(a, [1] * 6, h) for h in (10, 11, 51, 401, 0, 9)] == [vc.next_best_view(a, h) for h in (10, 11, 51, 401, 0, 9)]
    assert rc.next_reachable_view(a, [0] * 6, 0) == -1


def test_sizes(capi):
    """Two bytes per voxel of field, three of workspace (rounded up), two 64-bit words per brick of reach buffer; 0 for bad resolutions."""
    bricks = lambda r: -(-r[0] // 4) * -(-r[1] // 4) * -(-r[2] // 4)
    for r in ((1, 1, 1), (3, 3, 3), (19, 18, 13), (20, 18, 13), (300, 4, 5), (64, 64, 64), (512, 512, 512)):
        n = r[0] * r[1] * r[2]
        assert capi.clearance_bytes(r) == 2 * n
        assert 3 * n <= capi.clearance_workspace_bytes(r) < 3 * n + 256
        assert 16 * bricks(r) < capi.reach_bytes(r) <= 16 * bricks(r) + 4096 and capi.reach_bytes(r) % 8 == 0
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (4, 70000, 4), (4, 4, 70000)):
        assert capi.clearance_bytes(bad) == 0 and capi.clearance_workspace_bytes(bad) == 0 and capi.reach_bytes(bad) == 0, bad


def test_bindings_exist(capi):
    """The entry points of every layer: the library's symbols with their ctypes signatures, the orchestrator's C ABI and the methods of
    KinectFusion (ShardedKinectFusion inherits them; in shard mode they raise XsError — the GPU suite)."""
    pl = importlib.import_module("x-slam_amd.pipeline")
    sh = importlib.import_module("x-slam_amd.sharded")
    for n in ("xs_clearance_bytes", "xs_clearance_workspace_bytes", "xs_clearance_build", "xs_reach_bytes", "xs_reach_passable", "xs_reach_flood",
              "xs_reach_expand", "xs_reach_query"):
        assert n in capi._SIGS and hasattr(capi._lib, n), n
    for n in ("xs_kf_clearance_field", "xs_kf_reachable", "xs_kf_next_reachable_view"):
        assert n in pl._SIGS and hasattr(pl._lib, n), n
    assert (capi.CLEARANCE_MAX_RADIUS, capi.REACH_MAX_SEEDS, capi.REACH_MAX_SNAP) == (255, 64, 16) and capi.abi_version() == 3
    for cls in (pl.KinectFusion, sh.ShardedKinectFusion):
        assert callable(cls.clearance_field) and callable(cls.reachable) and callable(cls.next_reachable_view)
