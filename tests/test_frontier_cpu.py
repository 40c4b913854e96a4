"""CPU-only: the host's side of frontier clusters and proposed views — the scipy model the kernels are held to
against a scalar brute force, the scenes the GPU tests use, the host algebra of x-slam_amd/host/view_host.hpp under the sanitizers and its
numpy twins, the buffer sizes and the bindings."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import frontier_cases as fc
import reach_cases as rc

EPS = 2.0 ** -24                                                               # the relative error of one float32 rounding


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module("x-slam_amd.capi")


@pytest.mark.parametrize("res", [(7, 6, 5), (5, 4, 9)])
@pytest.mark.parametrize("cell", [0, 8])
def test_model_equals_brute_force(res, cell):
    """Padded shifts, scipy's labelling per cell block and bincount against per-voxel neighbour tests and a breadth-first search over the
    26 neighbours within the cell.  (5, 4, 9) at cell 8 has two cells along z."""
    for seed, p in ((19, (0.05, 0.9, 0.05)), (17, (0.3, 0.4, 0.3)), (3, (0.5, 0.5, 0.0))):
        states = rc.random_states(res, seed=seed, p=p)
        m, lab, rec = fc.model(states, cell)
        bm, blab, brec = fc.brute(states, cell)
        assert m.sum() > 5 and np.array_equal(m, bm)
        assert lab.dtype == np.uint32 and np.array_equal(lab, blab)
        assert rec.dtype == np.uint64 and np.array_equal(rec, brec)
        assert np.array_equal(lab != fc.NONE, m) and rec[:, 1].sum() == m.sum() and np.all(np.diff(rec[:, 0].astype(np.int64)) > 0)
        lin = fc.linear_index(m.shape)
        assert np.array_equal(lab[lin == lab], rec[:, 0])                        # the roots are the voxels labelled with their own index


def test_frontier_rule_edge_cases():
    """An all-FREE volume has no frontier (outside is not UNKNOWN); OCCUPIED and UNKNOWN voxels are never frontier; a diagonal UNKNOWN
    neighbour does not count; one UNKNOWN voxel in free space has its six face neighbours as frontier, one 26-connected cluster."""
    assert not fc.frontier(np.full((5, 5, 5), fc.FREE, np.uint8)).any()
    s = np.full((5, 5, 5), fc.FREE, np.uint8)
    s[2, 2, 2] = fc.UNKNOWN
    m, lab, rec = fc.model(s, 0)
    assert m.sum() == 6 and not m[2, 2, 2] and not m[1, 1, 2] and m[1, 2, 2] and m[2, 2, 3]
    assert len(rec) == 1 and rec[0, 0] == (1 * 5 + 2) * 5 + 2 and rec[0, 1] == 6 and fc.unpack_box(rec[0, 5]) == (1, 1, 1) and fc.unpack_box(rec[0, 6]) == (3, 3, 3)
    s[1, 2, 2] = fc.OCCUPIED
    assert fc.frontier(s).sum() == 5 and not fc.frontier(s)[1, 2, 2]
    s[:] = fc.UNKNOWN
    assert not fc.frontier(s).any()


def test_the_scenes_of_the_gpu_tests():
    """The figures the GPU tests rely on, on the model alone: the two random scenes at both resolutions (more than one cluster, more at
    cell 8 than at cell 0), the serpentine as one cluster of 20 voxels, the long thin volume, the pair across a tile corner."""
    counts = {}
    for res in ((20, 18, 13), (19, 18, 13)):
        for seed, p in ((19, (0.01, 0.97, 0.02)), (17, (0.3, 0.4, 0.3))):
            states = rc.random_states(res, seed=seed, p=p)
            n = [len(fc.model(states, cell)[2]) for cell in (0, 8, 16)]
            counts[(res, seed)] = (int(fc.frontier(states).sum()), n)
            assert n[0] > 1 and n[1] > n[0] and n[1] >= n[2] >= n[0], (res, seed, n)
    print(counts)
    a, b = counts[((20, 18, 13), 19)], counts[((19, 18, 13), 19)]
    assert (a[0], a[1][:2]) == (281, [24, 52]) and (b[0], b[1][:2]) == (259, [21, 44])
    for res in ((20, 18, 13), (19, 18, 13)):
        c = counts[(res, 17)]
        assert 1400 < c[0] < 1800 and c[1][0] == 2 and 20 <= c[1][1] <= 40
    states, path = rc.serpentine((8, 8, 8), z=5)
    states[6] = fc.UNKNOWN
    m, lab, rec = fc.model(states, 0)
    assert len(path) == 20 and m.sum() == 20 and all(m[z, y, x] for x, y, z in path) and len(rec) == 1 and rec[0, 1] == 20
    # its runs are two voxels apart: without the turns they are three clusters
    for x, y, z in path:
        if y % 2 == 0:
            m[z, y, x] = False
    assert len(fc.records(fc.labels(m, 0))) == 3
    s = np.full((5, 4, 300), fc.UNKNOWN, np.uint8)
    s[:, :2, :] = fc.FREE
    m, lab, rec = fc.model(s, 0)
    assert m.sum() == 1500 and m[:, 1, :].all() and len(rec) == 1 and rec[0, 0] == 300 and len(fc.model(s, 8)[2]) == 38
    for b, want in (((8, 8, 8), {0: 1, 8: 2, 16: 1}), ((9, 9, 9), {0: 2, 8: 2, 16: 2})):
        m = np.zeros((16, 16, 16), bool)
        m[7, 7, 7] = m[b[2], b[1], b[0]] = True
        assert {c: len(fc.records(fc.labels(m, c))) for c in (0, 8, 16)} == want


def test_host_algebra_in_numpy():
    """The numpy twins of view_host.hpp that the GPU tests hold the orchestrator to.  Bounds from the operation count (EPS = 2^-24): a
    direction is unit within 4 EPS (float64 throughout); a look-at rotation built in float64 is orthonormal to float64 accuracy (1e-14)
    and, rounded to float32, within 8 EPS (nine roundings of entries below 1: a dot product moves by at most 2 EPS); its optical axis is
    parallel to centroid - position within 2 EPS (a vector error of at most sqrt(3) EPS)."""
    for j in range(32):
        d = fc.direction(j)
        assert abs(np.linalg.norm(d) - 1.0) < 1e-14 and d[2] == 1.0 - 2.0 * fc.halton(j + 1, 2)
    assert [fc.halton(i, 2) for i in (1, 2, 3, 4)] == [0.5, 0.25, 0.75, 0.125] and abs(fc.halton(1, 3) - 1 / 3) < 1e-15
    cen = np.array([3.84, 1.2, 6.5], np.float32)
    down, side = np.array([0.0, 1.0, 0.0]), np.array([1.0, 0.0, 0.0])
    for j in range(32):
        pos = (cen + np.float32(1.5) * fc.direction(j).astype(np.float32)).astype(np.float32)
        dist = np.linalg.norm(pos.astype(np.float64) - cen)
        assert abs(dist - 1.5) <= 1.5 * 4 * EPS + 2 * np.sqrt(3.0) * EPS * (np.linalg.norm(cen) + 1.5)   # one product and one sum per axis
        R = fc.look_at(pos, cen, down, side)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-14 and np.linalg.det(R) > 0.999
        R32 = R.astype(np.float32).astype(np.float64)
        assert np.abs(R32.T @ R32 - np.eye(3)).max() <= 8 * EPS
        to = (cen.astype(np.float64) - pos) / dist
        assert np.linalg.norm(np.cross(R32[:, 2], to)) <= 2 * EPS and R32[:, 2] @ to > 0
    # the fallback hint: within 8.1 degrees of the view direction the side hint takes over, beyond it the hint holds
    for tilt, fallback in ((0.0, True), (0.14, True), (0.15, False)):
        R = fc.look_at(np.zeros(3), np.array([0.0, 1.0, tilt]), down, side)
        assert (abs(R[0, 1] - 1.0) < 1e-14) == fallback and (abs(R[0, 0] - 1.0) < 1e-14) == (not fallback)
    assert fc.look_at(np.zeros(3), np.zeros(3), down, side) is None and fc.look_at(np.zeros(3), [0, 0, 1], [0, 0, 1], [0, 0, 2]) is None
    # centroids and the voxel-centre round trip over the whole index range, at the test scenes' voxel sizes among others
    assert np.array_equal(fc.centroid(np.array([300, 1500, 224250, 1500, 3000, 0, 0, 0], np.uint64), 0.5), np.array([75.0, 0.75, 1.25], np.float32))
    v = np.arange(65536)
    for vs in (0.125, 0.12, 3.0 / 64.0, 0.005859375, 0.0117, 0.03, 1e-3, 0.7, 3.0):
        c = fc.voxel_centre(v, vs)
        assert c.dtype == np.float32 and np.array_equal(np.floor(c / np.float32(vs)).astype(np.int64), v), vs


def test_frontier_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/view_host.hpp's voxel_centre, frontier_centroid, halton, frontier_direction, frontier_standpoint, look_at and
    frontier_select compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/frontier_selftest.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "frontier_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(root, "x-slam_amd", "host"), os.path.join(root, "tests", "cxx", "frontier_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_sizes(capi):
    """8 bytes per brick of mask, 4 per voxel of labels, a workspace that grows with the record capacity; 0 for bad resolutions, among them
    one whose voxels a uint32 label cannot index."""
    for r in ((1, 1, 1), (3, 3, 3), (19, 18, 13), (300, 4, 5), (64, 64, 64), (512, 512, 512)):
        bricks = ((r[0] + 3) // 4) * ((r[1] + 3) // 4) * ((r[2] + 3) // 4)
        assert capi.frontier_mask_bytes(r) == 8 * bricks and capi.frontier_label_bytes(r) == 4 * r[0] * r[1] * r[2]
        w0, w1, w2 = (capi.frontier_workspace_bytes(r, c) for c in (0, 1, 4096))
        assert 64 <= w0 <= 4096 and w0 % 8 == 0 and w0 < w1 <= w0 + 64 and w1 < w2 <= w0 + 4096 * 32
        assert capi.frontier_workspace_bytes(r, -1) == 0
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (4, 70000, 4), (4, 4, 70000), (2048, 2048, 1024)):
        assert capi.frontier_mask_bytes(bad) == 0 and capi.frontier_label_bytes(bad) == 0 and capi.frontier_workspace_bytes(bad, 16) == 0, bad
    assert capi.frontier_label_bytes((2048, 2048, 1023)) == 4 * 2048 * 2048 * 1023


def test_bindings_exist(capi):
    """The entry points of every layer: the library's symbols with their ctypes signatures, the orchestrator's C ABI and the methods of
    KinectFusion (ShardedKinectFusion inherits them; in shard mode they raise XsError — the GPU suite)."""
    pl = importlib.import_module("x-slam_amd.pipeline")
    sh = importlib.import_module("x-slam_amd.sharded")
    for n in ("xs_frontier_mask_bytes", "xs_frontier_label_bytes", "xs_frontier_workspace_bytes", "xs_frontier_mask", "xs_frontier_label", "xs_frontier_clusters",
              "xs_frontier_expand"):
        assert n in capi._SIGS and hasattr(capi._lib, n), n
    for n in ("xs_kf_frontiers", "xs_kf_propose_views"):
        assert n in pl._SIGS and hasattr(pl._lib, n), n
    assert (capi.FRONTIER_NONE, capi.FRONTIER_RECORD_WORDS) == (0xFFFFFFFF, 8) and capi.abi_version() == 3
    for cls in (pl.KinectFusion, sh.ShardedKinectFusion):
        assert callable(cls.frontiers) and callable(cls.propose_views) and callable(cls.explore_step)
    for f in ("frontier_mask_bytes", "frontier_label_bytes", "frontier_workspace_bytes", "frontier_mask", "frontier_label", "frontier_clusters", "frontier_expand"):
        assert callable(getattr(capi, f)), f
