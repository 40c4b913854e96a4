"""CPU-only: the model the transform score is held to (tests/align_score_cases.py) against align_cases.evaluate, the condition on its cases,
the strided entries, the host algebra of x-slam_amd/host/align_search_host.hpp through the exported functions and under the sanitizers, the
whole search with the model as the scorer on the analytic fixture, and the bindings of every layer."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import align_cases as ac
import align_score_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pl():
    return importlib.import_module("x-slam_amd.pipeline")


@pytest.mark.parametrize("sshape", sc.SOURCE_SHAPES)
def test_model_agrees_with_the_alignment_model(sshape):
    """Every count, transform and min_weight: the kept set is align_cases.evaluate's for the same map, and the sum of r^2 lies within that
    evaluate's own bound of its sums32[27] (its real part differs from this model's only by products of two imaginary parts, and it
    squares in double where the contract here squares in float32: both inside the bound).  The gates add up; the miss keeps nothing."""
    for count in sc.INDEX_COUNTS:
        xyz, gt, src = sc.case(sshape, count)
        for name, m in sc.case_xforms(sshape).items():
            for mw in sc.MIN_WEIGHTS:
                ev = sc.expected(sshape, count, name, mw)
                ref = ac.evaluate(xyz, gt, src, ac.case_maps(sshape)[name], mw)
                assert np.array_equal(ev["kept"], ref["kept"]), (count, name, mw)
                assert ev["count"] == ref["sums32"][28] == ev["kept"].sum()
                assert abs(ev["sum"] - ref["sums32"][27]) <= ref["bound"][27], (count, name, mw, ev["sum"], ref["sums32"][27], ref["bound"][27])
                assert (ev["outside"], ev["weight"], ev["residual"]) == (ref["outside"], ref["weight"], ref["residual"])
                assert ev["outside"] + ev["weight"] + ev["residual"] + ev["count"] == count
                assert ev["terms"].dtype == np.float32 and (ev["terms"] >= 0).all() and not ev["terms"][~ev["kept"]].any()
                if name == "miss":
                    assert ev["outside"] == count and ev["sum"] == 0.0


@pytest.mark.parametrize("sshape", sc.SOURCE_SHAPES)
def test_condition_on_the_cases(sshape):
    """No case has an entry inside the margin of max_residual; every case of 255 entries or more drops entries at each of the three gates
    and keeps some, over its transforms and min_weights together."""
    for count in sc.INDEX_COUNTS:
        xyz, gt, src = sc.case(sshape, count)
        full, near = sc.condition(xyz, gt, src, sshape)
        assert near == 0, count
        if count >= sc.FULL_CASE_COUNT:
            assert full, count
    if sshape == (9, 10, 13):
        xyz, gt, src = sc.large_case()
        assert sc.condition(xyz, gt, src, sshape) == (True, 0) and len(gt) == 300000 > 1024 * 4 * 64


def test_strided_entries():
    """Stride s scores entries 0, s, 2 s, ...: ceil(count / s) of them, the model run on xyz[::s]."""
    sshape = (9, 10, 13)
    for count in (1, 64, 65, 257):
        xyz, gt, src = sc.case(sshape, count)
        whole = sc.expected(sshape, count, "rotation_7", 1)
        for s in sc.STRIDES:
            sx, sg = sc.strided(xyz, gt, s)
            assert len(sg) == -(-count // s) and np.array_equal(sx, xyz[np.arange(0, count, s)])
            ev = sc.expected(sshape, count, "rotation_7", 1, s)
            assert np.array_equal(ev["kept"], whole["kept"][::s]) and np.array_equal(ev["terms"].view(np.uint32), whole["terms"][::s].view(np.uint32))
            assert ev["count"] == whole["kept"][::s].sum()


def test_free_candidates(pl):
    """Rotations orthonormal with determinant +1 to 1e-12, this map's centroid mapped to within box_t sqrt(3) of the other's, the sequence
    a prefix of itself, and the refusals."""
    ct, co, box = np.array([2.41, 2.33, 2.87]), np.array([2.2, 2.6, 2.1]), 0.3
    T = pl.transform_candidates_free(2048, ct, co, box)
    assert T.shape == (2048, 4, 4) and T.dtype == np.float64
    R = T[:, :3, :3]
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12 and np.abs(np.linalg.det(R) - 1.0).max() <= 1e-12
    assert np.array_equal(T[:, 3], np.tile([0.0, 0, 0, 1], (2048, 1)))
    d = np.linalg.norm(T[:, :3, :3] @ ct + T[:, :3, 3] - co, axis=1)
    assert d.max() <= box * np.sqrt(3) and d.max() > 0.5 * box
    assert np.array_equal(pl.transform_candidates_free(7, ct, co, box), T[:7])
    # the Halton points, restated: candidate i's jitter is box (2 halton(i + 1; 7, 11, 13) - 1)
    for i in (0, 1, 50, 2047):
        want = box * (2 * np.array([pl._halton(i + 1, b) for b in (7, 11, 13)]) - 1)
        assert np.abs(T[i, :3, :3] @ ct + T[i, :3, 3] - co - want).max() < 1e-12
    # the rotations are spread out: no two of the first 256 closer than 5 degrees, every rotation of a sample within 40 of a candidate
    tr = np.einsum("iab,jab->ij", R[:256], R[:256])
    ang = np.degrees(np.arccos(np.clip(0.5 * (tr - 1), -1, 1)))
    assert ang[~np.eye(256, dtype=bool)].min() > 5.0
    for bad in (dict(n=0), dict(box_t=-0.1), dict(box_t=np.nan), dict(centroid_this=[np.inf, 0, 0]), dict(centroid_other=[0, np.nan, 0])):
        args = dict(n=4, centroid_this=ct, centroid_other=co, box_t=box)
        args.update(bad)
        with pytest.raises(ValueError):
            pl.transform_candidates_free(**args)


def test_candidates_around(pl):
    """Entry 0 is T bit for bit; every entry moves the pivot's image by at most box_t sqrt(3) and turns by at most box_r sqrt(3)."""
    rng = np.random.default_rng(71)
    for it in range(20):
        T = np.eye(4)
        T[:3, :3] = ac.rotation(rng.normal(size=3), rng.uniform(-3, 3))
        T[:3, 3] = rng.uniform(-3, 3, 3)
        pivot, bt, br = rng.uniform(0, 5, 3), rng.uniform(0, 0.5), rng.uniform(0, 0.5)
        out = pl.transform_candidates_around(T, pivot, bt, br, 256)
        assert out.shape == (256, 4, 4) and np.array_equal(out[0].view(np.uint64), T.view(np.uint64))
        q = T[:3, :3] @ pivot + T[:3, 3]
        moved = np.linalg.norm(out[:, :3, :3] @ pivot + out[:, :3, 3] - q, axis=1)
        assert moved.max() <= bt * np.sqrt(3) + 1e-12
        rel = out[:, :3, :3] @ T[:3, :3].T
        assert np.abs(rel @ rel.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-12
        ang = np.arccos(np.clip(0.5 * (np.trace(rel, axis1=1, axis2=2) - 1), -1, 1))
        assert ang.max() <= br * np.sqrt(3) + 1e-7
        if it == 0:
            assert moved.max() > 0.5 * bt and ang.max() > 0.5 * br
            # restated: entry i is exp(box_r u[3:6]) about q, then box_t u[0:3]
            for i in (1, 2, 77):
                u = 2 * np.array([pl._halton(i, b) for b in (2, 3, 5, 7, 11, 13)]) - 1
                E = ac.se3_exp(np.concatenate([np.zeros(3), br * u[3:]]))[:3, :3]
                assert np.abs(out[i, :3, :3] - E @ T[:3, :3]).max() < 1e-12
                assert np.abs(out[i, :3, 3] - (E @ (T[:3, 3] - q) + q + bt * u[:3])).max() < 1e-12
    for bad in (dict(n=0), dict(box_t=-1.0), dict(box_r=-1.0), dict(box_r=np.inf), dict(T=np.full((4, 4), np.nan)), dict(pivot=[0, 0, np.nan])):
        args = dict(T=np.eye(4), pivot=np.zeros(3), box_t=0.1, box_r=0.1, n=3)
        args.update(bad)
        with pytest.raises(ValueError):
            pl.transform_candidates_around(**args)


def test_rank_against_a_stable_sort(pl):
    """The keep best by S = count - sum r^2, ties to the lower index: numpy's stable argsort of -S."""
    rng = np.random.default_rng(73)
    for it in range(100):
        P, keep = int(rng.integers(1, 80)), int(rng.integers(1, 40))
        out = np.stack([0.25 * rng.integers(0, 4, P), rng.integers(0, 6, P).astype(np.float64)], axis=1)     # many ties
        want = np.argsort(-(out[:, 1] - out[:, 0]), kind="stable")[:keep]
        assert np.array_equal(pl.transform_rank(out, keep), want), it
    assert len(pl.transform_rank(np.zeros((3, 2)), 0)) == 0


def test_band_centroid_against_exact_integers(pl):
    rng = np.random.default_rng(79)
    for n in (1, 2, 1000):
        xyz = np.stack([rng.integers(0, 2 ** 21, n), rng.integers(0, 2 ** 21, n), rng.integers(0, 2 ** 22, n)], axis=1).astype(np.int64)
        got = pl.band_centroid(ac.keys_of(xyz), 0.05)
        for a in range(3):
            total = sum(int(v) for v in xyz[:, a])
            assert got[a] == (total / n + 0.5) * 0.05
    with pytest.raises(ValueError):
        pl.band_centroid(np.zeros(0, np.int64), 0.05)


def test_fixture_is_the_scene_it_says():
    """The band of this map holds the voxel count the feasibility study of DESIGN.md section 4.24 was run on; the other map is the same
    field: its values at the images of this map's voxel centres agree with this map's to the interpolation error of a 0.1 m grid."""
    v, w = sc.scene_volume()
    xyz, gt = ac.band_of(v)
    assert len(gt) == sc.SCENE_BAND_VOXELS and v.shape == (48, 48, 48) and set(np.unique(w)) == {0, 1} and not v[w == 0].any()
    for deg in (35, 100, 170):
        other = sc.scene_volume(deg)
        assert other[1].sum() > 50000 and not other[0][other[1] == 0].any()


def test_search_on_the_model_reaches_the_truth(pl):
    """The whole search with the model as the scorer, 35 degrees: 1024 candidates, stride 8, keep 8, 2 rounds, box 0.3 m, refinement boxes
    0.25 m / 0.25 rad, then align_cases.loop with 10 iterations on the best four.  Each of the four ends within 0.01 voxel in corner
    displacement of the loop started at T_true (the margin tests/test_align_pipeline_gpu.py allows against its truth) and with at least
    0.98 of its S.  Observed when this was written: see DESIGN.md section 4.24; the values are printed."""
    vs, deg = sc.SCENE_VS, 35
    this, other = sc.scene_volume()[0], sc.scene_volume(deg)
    T_true = sc.scene_truth(deg)
    log = []
    kept, S = sc.search_on_the_model(this, other, vs, 1024, 8, 2, 8, 0.3, 0.25, 0.25, pl, log=log)
    best_per_round = [float(s.max()) for _, s in log] + [float(S.max())]
    assert all(b >= a for a, b in zip(best_per_round, best_per_round[1:])), best_per_round       # a kept transform re-enters its own group
    xyz, gt = ac.band_of(this)
    ok, T_ref, _, ev = ac.loop(xyz, gt, other, T_true, vs, vs, 10)
    assert ok
    S_ref = ev["sums32"][28] - ev["sums32"][27]
    res = (sc.SCENE_N,) * 3
    print("reference: S", S_ref, "count", ev["sums32"][28], "truth to its own minimum (m)", ac.corner_displacement(T_ref, T_true, res, vs))
    print("kept after the last round: S (strided)", S, "corner displacement (m)", [ac.corner_displacement(T, T_true, res, vs) for T in kept])
    for k in range(4):
        ok, T, _, ev = ac.loop(xyz, gt, other, kept[k], vs, vs, 10)
        d, Sk = ac.corner_displacement(T, T_ref, res, vs), ev["sums32"][28] - ev["sums32"][27]
        print("start", k, "ends", d, "m from the reference, S", Sk)
        assert ok and d <= 0.01 * vs and Sk >= 0.98 * S_ref, (k, d, Sk, S_ref)


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/align_search_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run
    (tests/cxx/align_search_selftest.cpp)."""
    exe = str(tmp_path / "align_search_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "x-slam_amd", "host"), os.path.join(ROOT, "tests", "cxx", "align_search_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_sizes_and_bindings(pl):
    """Tickets, 4096 maps of 12 floats and 1024 records of 64 doubles + 64 counts per tile of 64 transforms; 0 outside 1 .. 4096; the entry
    points of every layer; the options' defaults."""
    capi = importlib.import_module("x-slam_amd.capi")
    sh = importlib.import_module("x-slam_amd.sharded")
    for n, tiles in ((1, 1), (64, 1), (65, 2), (4096, 64)):
        assert capi.tsdf_score_transforms_workspace_bytes(n) == 256 + 4096 * 48 + tiles * 1024 * 64 * 12
    for n in (0, -1, 4097):
        assert capi.tsdf_score_transforms_workspace_bytes(n) == 0
    assert capi.ALIGN_SCORE_MAX_TRANSFORMS == sc.MAX_TRANSFORMS == 4096
    for n in ("xs_tsdf_score_transforms", "xs_tsdf_score_transforms_workspace_bytes"):
        assert n in capi._SIGS and hasattr(capi._lib, n), n
    for n in ("xs_kf_score_transforms", "xs_kf_score_transforms_checkpoint", "xs_kf_align_map_global", "xs_kf_align_checkpoint_global",
              "xs_kf_align_search_defaults", "xs_host_align_search_free", "xs_host_align_search_around", "xs_host_align_search_rank", "xs_host_band_centroid"):
        assert n in pl._SIGS and hasattr(pl._lib, n), n
    for cls in (pl.KinectFusion, sh.ShardedKinectFusion):
        assert callable(cls.score_transforms) and callable(cls.align_map_global) and callable(cls.align_checkpoint_global)
        assert "merge_checkpoint(path, kf.align_checkpoint_global(path)[1])" in cls.align_checkpoint_global.__doc__
        assert "symmetr" in cls.align_map_global.__doc__
    assert callable(pl.transform_candidates_free) and callable(pl.transform_candidates_around) and callable(capi.tsdf_score_transforms)
    import ctypes as C
    assert C.sizeof(pl.AlignSearchOpts) == 80
    # the host entries refuse null pointers without touching anything
    assert pl._lib.xs_host_align_search_free(3, None, None, 0.1, None) == -1 and pl._lib.xs_host_align_search_around(None, None, 0.1, 0.1, 3, None) == -1
    assert pl._lib.xs_host_align_search_rank(None, 3, 2, None) == 0 and pl._lib.xs_host_band_centroid(None, 3, 0.1, None) == -1
