"""CPU: the cases and the model that hold xs_tsdf_score_points and register_points_global (tests/register_score_cases.py; DESIGN.md section
4.32), the host's side of the search (register_search_host.hpp) through its C ABI and under the sanitizers, and the whole search on the model."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import align_cases as ac
import align_score_cases as asc
import register_cases as rg
import register_score_cases as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = rs.cases() + (rs.big_case(),)


@pytest.fixture(scope="module")
def pl():
    return importlib.import_module("x-slam_amd.pipeline")


def test_conditions_on_the_cases():
    """Every (case, stride) with 255 scored points or more: each of the three gates drops a point, a point is kept; no (case, stride) at all has
    an |r| within 2^-22 of max_residual without equalling it; points exactly at +-max_residual exist in the identity cases and are kept."""
    full, planted = 0, 0
    for case in ALL_CASES:
        for stride in rs.STRIDES:
            ev = rs.expected(case["name"], stride)
            n = case["n"]
            assert ev["scored"] == -(-n // stride) and ev["near"] == 0, (case["name"], stride, ev["near"])
            assert ev["outside"] + ev["unseen"] + ev["residual"] + ev["count"] == ev["scored"]
            if ev["scored"] >= rs.FULL_CASE_COUNT:
                full += 1
                assert min(ev["outside"], ev["unseen"], ev["residual"], ev["count"]) > 0, (case["name"], stride, ev["outside"], ev["unseen"], ev["residual"], ev["count"])
            if case.get("planted") is not None and case["n"] >= rs.FULL_CASE_COUNT and stride == 1:
                planted += 1
                assert ev["equal"] >= 6, (case["name"], ev["equal"])
            print(case["name"], "stride", stride, "scored", ev["scored"], "outside", ev["outside"], "unseen", ev["unseen"], "residual", ev["residual"], "kept", ev["count"],
                  "equal", ev["equal"])
    assert full >= 10 and planted == 2
    # the large case at the GPU test's stride: more chunks than one round of the grid takes
    big = next(c for c in ALL_CASES if c["n"] == rg.BIG_N)
    assert -(-(rg.BIG_N // 4) // 64) == 4160 > 4 * rs.MAX_BLOCKS and rs.nblocks_of(rg.BIG_N // 4) == rs.MAX_BLOCKS and big["tile"] == 256


def test_a_point_may_count_here_that_register_terms_drops():
    """No gradient gate: the kept set contains register_terms' kept set at stride 1, and in some case it is strictly larger."""
    larger = 0
    for case in rs.cases():
        ev, terms = rs.expected(case["name"]), rg.expected(case["name"])["point"]
        assert not (terms["kept"] & ~ev["kept"][:len(terms["kept"])]).any(), case["name"]
        larger += int((ev["kept"][:len(terms["kept"])] & ~terms["kept"]).sum())
    assert larger > 0


@pytest.mark.parametrize("mutant", rs.MUTANTS)
def test_mutants_change_a_pair(mutant):
    """Each mutant moves the pair of some (case, stride) beyond the GPU test's tolerance (count unequal, or the sum off by more than 8 u sum)."""
    pool = [rs.wrap_case()] if mutant == "row_wrap32" else [c for c in ALL_CASES if c["n"] < rg.BIG_N]
    hits = []
    for case in pool:
        for stride in rs.STRIDES:
            good = rs.score_model(case, case["xform"], stride)
            if rs.differs(good, rs.score_model(case, case["xform"], stride, mutant)):
                hits.append((case["name"], stride))
    assert hits, mutant
    if mutant in ("stride_last", "stride_ignored"):
        assert all(s > 1 for _, s in hits)
    print(mutant, "changes", len(hits), "pairs, e.g.", hits[:3])


def test_score_many_is_the_model():
    """The batched scorer of the search fixture gives score_model's pairs bit for bit, on a case's transforms and strides."""
    case = next(c for c in rs.cases() if c["name"] == "sphere_n257_rigid_mw3_mr03")
    X = rs.transforms(case, 9)
    for stride in rs.STRIDES:
        many = rs.score_many(case["vol"], case["vs"], rg.all_points(case), X, stride, case["min_weight"], case["max_residual"], case["pitch"], batch=4)
        for p in range(len(X)):
            ev = rs.score_model(case, X[p], stride)
            assert many[p, 0] == ev["sum"] and many[p, 1] == ev["count"], (stride, p)
        assert many[1, 1] == 0 and (stride > 1 or many[0, 1] > 0)      # (transform 1 maps every point outside)


def test_points_centroid_against_numpy(pl):
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, 1000):
        p = rng.uniform(-5, 5, (n, 3)).astype(np.float32)
        for stride in (1, 2, 3, 7, 2000):
            got = pl.points_centroid(p, stride)
            q = p[::stride].astype(np.float64)
            want = np.array([np.add.accumulate(q[:, a])[-1] for a in range(3)]) / len(q)      # index order
            assert np.array_equal(got, want), (n, stride)
    with pytest.raises(ValueError):
        pl.points_centroid(np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError):
        pl.points_centroid(np.zeros((4, 3), np.float32), 0)


def test_fixture_is_the_cloud_it_says(pl):
    """The deterministic cloud: its sizes, every point on the scene's surface and inside the map's seen band, the half cloud's centroid 0.84 m
    from the map's band centroid, and at the answer nearly every point kept with a small residual."""
    pm, half = rs.scene_cloud(), rs.scene_cloud(True)
    assert len(pm) == rs.SCENE_CLOUD_POINTS and len(half) == rs.SCENE_HALF_POINTS
    assert np.abs(asc.scene_sdf(pm)).max() < 1e-9 and pm.min() > 0.15 and pm.max() < 4.65
    c_map = rs.map_band_centroid(asc.scene_volume()[0], asc.SCENE_VS, pl)
    off = float(np.linalg.norm(half.mean(axis=0) - c_map))
    assert 0.80 < off < 0.88, off
    case = rs.scene_case()
    for deg in (100, 170):
        cloud, T = rs.handed_cloud(deg)
        ev = rs.score_model(case, rg.xform12_of(T), 1, pts=cloud)
        assert ev["count"] >= 0.99 * len(cloud) and ev["sum"] / ev["count"] < 0.02, (deg, ev["count"], ev["sum"])


@pytest.mark.parametrize("deg,half", [(100, False), (100, True)], ids=["full_100", "half_100"])
def test_search_on_the_model_reaches_the_truth(pl, deg, half):
    """The whole search at register_points_global's defaults (2048 candidates, stride 4, keep 8, 2 rounds, boxes 0.3 m / 0.25 rad) with the float32
    model as the scorer, then register_cases' model loop (10 iterations) from every kept transform: the one with the highest S among those that
    ended ok lies within 0.01 voxel of worst-corner displacement of the model loop started at the truth and reaches 0.98 of its S.  The values are
    printed; DESIGN.md section 4.32 records them."""
    vs, res = asc.SCENE_VS, (asc.SCENE_N,) * 3
    case, vol = rs.scene_case(), asc.scene_volume()
    cloud, T_true = rs.handed_cloud(deg, half)
    log = []
    kept, S = rs.search_on_the_model(cloud, vol, vs, 2048, 8, 2, 4, asc.SCENE_TRUNC, asc.SCENE_TRUNC, 0.25, pl, log=log)
    best_per_round = [float(s.max()) for _, s in log] + [float(S.max())]
    assert all(b >= a for a, b in zip(best_per_round, best_per_round[1:])), best_per_round       # a kept transform re-enters its own group
    ok, T_ref, _, s_ref = rg.loop(case, cloud, T_true, 10)
    assert ok
    S_ref = s_ref[28] - s_ref[27]
    print("reference: S", S_ref, "count", s_ref[28], "truth to its own minimum (m)", ac.corner_displacement(T_ref, T_true, res, vs))
    print("kept after the last round: S (strided)", S, "corner displacement (m)", [round(ac.corner_displacement(T, T_true, res, vs), 3) for T in kept])
    ends = []
    for k in range(len(kept)):
        ok, T, _, s = rg.loop(case, cloud, kept[k], 10)
        d, Sk = ac.corner_displacement(T, T_ref, res, vs), s[28] - s[27]
        print("start", k, "ok", ok, "ends", d, "m from the reference, S", Sk)
        if ok:
            ends.append((Sk, -k, d))
    assert ends
    Sk, _, d = max(ends)
    assert d <= rs.SEARCH_AGREEMENT_VOXELS * vs and Sk >= rs.SEARCH_S_FRACTION * S_ref, (d, Sk, S_ref)


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/register_search_host.hpp and register_host.hpp's scoring table compiled with -fsanitize=address,undefined
    -fno-sanitize-recover and run as a stand-alone program (tests/cxx/register_search_selftest.cpp)."""
    exe = str(tmp_path / "register_search_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "x-slam_amd", "host"), os.path.join(ROOT, "tests", "cxx", "register_search_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_sizes_and_bindings(pl):
    """Tickets, 4096 transforms of 12 floats and 1024 records of 64 doubles + 64 counts per tile of 64 transforms; 0 outside 1 .. 4096; the entry
    points of every layer; the options struct's size and the Python defaults.  (The options' refusal table is the selftest's above: it needs
    no instance there.)"""
    capi = importlib.import_module("x-slam_amd.capi")
    for n, tiles in ((1, 1), (64, 1), (65, 2), (4096, 64)):
        assert capi.tsdf_score_points_workspace_bytes(n) == 256 + 4096 * 48 + tiles * 1024 * 64 * 12
    for n in (0, -1, 4097):
        assert capi.tsdf_score_points_workspace_bytes(n) == 0
    assert capi.REGISTER_SCORE_MAX_TRANSFORMS == rs.MAX_TRANSFORMS
    for name in ("score_point_transforms", "score_map_point_transforms", "score_checkpoint_point_transforms", "register_points_global",
                 "register_map_points_global", "register_checkpoint_points_global"):
        assert callable(getattr(pl.KinectFusion, name)), name
    import ctypes as C
    assert C.sizeof(pl.RegisterSearchOpts) == C.sizeof(pl.AlignSearchOpts) == 80
    import inspect
    assert inspect.signature(pl.KinectFusion.register_and_fuse).parameters["global_search"].default is False
    assert inspect.signature(pl.KinectFusion.register_points_global).parameters["max_residual"].default == 0.9
