"""CPU: the cases and models of tests/fuse_cases.py held to the conditions the GPU tests rely on (xs_tsdf_fuse_points_accumulate and
xs_tsdf_fuse_points_fold, x-slam_amd/csrc/xs_fuse.hip): the case set, the float64 twin within the derived bound, no
forbidden near miss, every mutant visible, the order of the points immaterial, the host header under the sanitizers, the bindings of every layer,
and the accuracy of the fused surface on an analytic scene."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import fuse_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = fc.all_cases()
F32, F64 = np.float32, np.float64


def test_the_case_set_is_the_issues():
    names = [c["name"] for c in ALL]
    assert len(set(names)) == len(names)
    combos = {(c["shape"], c["carve"], c["xform"] is not None, c["obs_weight"]) for c in fc.cases()}
    for shape in ((2, 2, 2), (5, 3, 2), (70, 9, 11)):
        for carve in (False, True):
            for rigid in (False, True):
                for ws in (1, 3):
                    assert (shape, carve, rigid, ws) in combos
    assert all(c["max_weight"] == 4 and c["pitch"] > c["shape"][0] * 4 for c in fc.cases())
    assert any(c["launches"] == 2 for c in ALL) and fc.hot_case()["n"] == 70000 and fc.big_case()["shape"] == (65, 33, 64)
    for c in fc.cases():
        X, Y, Z = c["shape"]
        ov = (c["T"][:3, :3] @ c["origin"].astype(F64) + c["T"][:3, 3]) / float(c["vs"])           # the origin in the volume frame, in voxels
        assert ((ov > 0) & (ov < (X, Y, Z))).all() == (c["obs_weight"] == 1 or c["launches"] == 2), (c["name"], ov)   # a sensor inside, and one outside
        p = c["pts"]
        assert np.isnan(p).any() and np.isinf(p).any() and (p == c["origin"]).all(axis=1).any(), c["name"]


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_conditions(case):
    """Every non-degenerate case: at least 50 voxels visited twice or more, at least 50 written over a weight > 0, points dropped and points used,
    samples outside, the weight cap acting where obs_weight is 3.  The hot voxel: a count past 2^16 and a sum past 2^32 in one word.  The big case: at
    least 50 voxels written in rows past 2^31 bytes."""
    ev = fc.expected(case["name"])
    cnt, s = ev["acc"] >> fc.COUNT_SHIFT, ev["acc"] & fc.SUM_MASK
    wp = np.array(case["vol"][1])
    assert int(cnt.sum()) == int(ev["counts"][2]) and ev["written"] == int((cnt > 0).sum()) and not ev["acc_after"].any()
    assert int(ev["counts"][0] + ev["counts"][1]) == case["n"]
    assert (s <= cnt * np.uint64(65536)).all()
    if not case["degenerate"]:
        assert int((cnt >= 2).sum()) >= 50 and int(((cnt > 0) & (wp > 0)).sum()) >= 50, case["name"]
        assert ev["counts"][0] > 0 and ev["counts"][3] > 0
        if case["name"] != "big_rows":
            assert ev["counts"][1] > 0
        if case["obs_weight"] == 3:
            assert int(((cnt > 0) & (wp + 3 > 4)).sum()) >= 50 and int(ev["vol"][1].max()) == 4
    if case["name"] == "hot_voxel":
        assert int(cnt.max()) == 70000 > 2 ** 16 and int(s.max()) == 70000 * 65536 > 2 ** 32
    if case["name"] == "big_rows":
        assert fc.high_rows_written(case, ev) >= 50
    # the untouched voxels keep their bits
    t = cnt > 0
    for before, after in zip(case["vol"], ev["vol"]):
        assert np.array_equal(np.array(before)[~t].view(np.uint32), after[~t].view(np.uint32))


def test_special_rays_do_what_they_are_there_for():
    """On the lattice cases: rays along each axis in both directions are used and put samples exactly on voxel faces; a voxel centre exactly
    tranc_dist behind a point gets q == 0 (u == -1.0f is kept); rays shorter than the band start at the sensor; some rays leave the volume inside
    their band."""
    for case in fc.cases():
        w = fc.expected(case["name"])["walk"]
        K = fc.half_steps(case)
        assert K == (8 if case["lattice"] else 7)
        if case["shape"] != (70, 9, 11):
            continue
        first = np.array([w["k"][w["pt"] == p].min() if (w["pt"] == p).any() else K + 1 for p in range(w["n"])])
        assert ((first > -K) & w["used"]).sum() >= 4 or case["carve"], case["name"]          # k_far < K: the ray starts at the sensor
        last_inside = np.array([w["inside"][(w["pt"] == p) & (w["k"] == K)].any() for p in range(w["n"])])
        assert (w["used"] & ~last_inside).sum() >= 10                                         # the band's far end lies outside the volume
        if case["lattice"]:
            on_face = w["inside"] & (w["g"] == np.floor(w["g"])).any(axis=1)
            assert on_face.sum() >= 10, case["name"]
            if case["obs_weight"] == 1:
                assert (w["visit"] & (w["u"] == F32(-1))).sum() >= 3 and (w["q"][w["visit"] & (w["u"] == F32(-1))] == 0).all(), case["name"]
        if case["lattice"] and case["obs_weight"] == 1:
            d = w["pt"][w["visit"]]
            axes = 0
            for p in range(w["n"]):
                v = case["pts"][p] - case["origin"]
                if w["used"][p] and (v != 0).sum() == 1 and (d == p).any():
                    axes |= 1 << (2 * int(np.nonzero(v)[0][0]) + int(v.sum() > 0))
            assert axes == 63, (case["name"], axes)


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_model_agrees_with_its_float64_twin(case):
    """V's a is the float32 walk bit for bit and its b the float64 operations on the model's decisions; |a - b| <= e for L, every g and every u;
    no ray of the case has a forbidden near miss; so the twin's own decisions, taken freely, are the model's, and its q differs nowhere."""
    w = fc.expected(case["name"])["walk"]
    rp = fc.replay(case, w)
    fin = np.isfinite(rp["L"].a) & np.isfinite(rp["L"].b)
    assert np.array_equal(rp["L"].a.view(np.uint32), w["L"].view(np.uint32))
    assert (np.abs(rp["L"].a[fin].astype(F64) - rp["L"].b[fin]) <= rp["L"].e[fin]).all()
    for c in range(3):
        g = rp["g"][c]
        assert np.array_equal(g.a.view(np.uint32), w["g"][:, c].view(np.uint32))
        assert (np.abs(g.a.astype(F64) - g.b) <= g.e).all()
    r = rp["reached"]
    assert np.array_equal(rp["u"].a.view(np.uint32), w["u"][r].view(np.uint32)) and np.array_equal(rp["qf"].a.view(np.uint32), w["qf"][r].view(np.uint32))
    assert (np.abs(rp["u"].a.astype(F64) - rp["u"].b) <= rp["u"].e).all()
    bad, kinds = fc.near_misses(case, w, rp)
    assert not bad.any(), (case["name"], kinds)
    w64 = fc.walk(case, np.float64)
    assert np.array_equal(w64["used"], w["used"]) and len(w64["pt"]) == len(w["pt"])
    for k in ("pt", "k", "inside", "i", "reached", "visit", "q"):
        assert np.array_equal(w64[k], w[k]), (case["name"], k)
    assert np.array_equal(w64["u"][r], rp["u"].b) and np.array_equal(w64["L"][fin], rp["L"].b[fin])
    worst = float(np.abs(rp["u"].a.astype(F64) - rp["u"].b).max()) if len(r) else 0.0
    print(case["name"], "largest |u32 - u64| %.3g, largest bound %.3g, samples %d, visits %d" % (worst, float(rp["u"].e.max()) if len(r) else 0.0, len(w["pt"]), int(w["visit"].sum())))


@pytest.mark.parametrize("mutant", fc.MUTANTS)
def test_every_mutant_changes_an_expected_byte(mutant):
    hit = [c["name"] for c in ALL if not fc.same_bytes(fc.evaluate(c, mutant)["vol"], fc.expected(c["name"])["vol"])]
    assert hit, mutant
    print(mutant, "changes", len(hit), "of", len(ALL), "cases")


def test_the_order_of_the_points_does_not_matter():
    """The points reversed and shuffled: equal accumulator words, counts and volumes.  (np.add.at on uint64: integer addition has no order.)"""
    for case in fc.cases():
        want = fc.expected(case["name"])
        for order in (np.arange(len(case["pts"]))[::-1], np.random.default_rng(3).permutation(len(case["pts"]))):
            c = dict(case, pts=case["pts"][order])
            ev = fc.evaluate(c)
            assert fc.same_bytes(ev["acc"], want["acc"]) and fc.same_bytes(ev["vol"], want["vol"]) and np.array_equal(ev["counts"], want["counts"]), case["name"]


def test_several_accumulates_before_one_fold():
    case = next(c for c in ALL if c["launches"] == 2)
    cut = fc.launch_split(case)
    acc = None
    for a, b in zip(cut[:-1], cut[1:]):
        part = dict(case, pts=case["pts"][a:b])
        acc = fc.accumulate(part, fc.walk(part), acc)
    assert fc.same_bytes(acc, fc.expected(case["name"])["acc"])


def test_fold_plane_range_and_second_sweep():
    """Planes outside [z0, z1) keep their voxels AND their words; folding the rest afterwards gives the whole fold; a second sweep over the result
    averages by the running mean with the grad scaled again."""
    case = next(c for c in ALL if c["name"] == "v70x9x11_carve_rigid_w1")
    want = fc.expected(case["name"])
    vol, acc, n1 = fc.fold(case["vol"], want["acc"], 1, 4, 3, 7)
    assert acc[:3].any() and acc[7:].any() and not acc[3:7].any()
    for before, after in zip(case["vol"], vol):
        assert np.array_equal(np.array(before)[:3], after[:3]) and np.array_equal(np.array(before)[7:], after[7:])
    vol, acc, n2 = fc.fold(vol, acc, 1, 4, 0, 3)
    vol, acc, n3 = fc.fold(vol, acc, 1, 4, 7, 11)
    assert fc.same_bytes(vol, want["vol"]) and n1 + n2 + n3 == want["written"] and not acc.any()
    again, _, _ = fc.fold(vol, want["acc"], 1, 4)
    t = (want["acc"] >> fc.COUNT_SHIFT) > 0
    o = (((want["acc"] & fc.SUM_MASK).astype(F64) / np.maximum(want["acc"] >> fc.COUNT_SHIFT, 1).astype(F64)) * 2.0 ** -15 - 1.0)
    wp = vol[1][t].astype(F64)
    assert np.allclose(again[0][t], (vol[0][t] * wp + o[t]) / (wp + 1), atol=1e-6) and np.allclose(again[2][t], vol[2][t] * wp / (wp + 1), atol=1e-6)
    assert (again[2][t & (np.array(case["vol"][1]) == 0)] == 0).all()


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/fuse_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/fuse_selftest.cpp)."""
    exe = str(tmp_path / "fuse_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "x-slam_amd", "host"), os.path.join(ROOT, "tests", "cxx", "fuse_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_sizes_and_bindings():
    """8 bytes per voxel, 0 for an unusable resolution; the entry points of every layer, in headers, libraries and tables; the limits agree."""
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    assert capi.fuse_accumulator_bytes([70, 9, 11]) == 70 * 9 * 11 * 8 and capi.fuse_accumulator_bytes([512, 512, 512]) == 1 << 30
    assert capi.fuse_accumulator_bytes([0, 9, 11]) == 0 and capi.fuse_accumulator_bytes(None) == 0
    assert capi.FUSE_MAX_POINTS == fc.MAX_POINTS and capi.FUSE_MAX_HALF_STEPS == fc.MAX_HALF_STEPS
    import ctypes
    assert ctypes.sizeof(capi.FuseOpts) == 16 and capi.fuse_opts().struct_bytes == 16
    with open(os.path.join(ROOT, "include", "xslam_amd.h")) as f:
        h = f.read()
    with open(os.path.join(ROOT, "include", "xslam_amd_pipeline.h")) as f:
        hp = f.read()
    for name in ("xs_tsdf_fuse_accumulator_bytes", "xs_tsdf_fuse_points_accumulate", "xs_tsdf_fuse_points_fold", "XS_FUSE_MAX_HALF_STEPS 256", "xs_fuse_opts"):
        assert name in h, name
    for name in ("xs_kf_fuse_points", "xs_kf_release_fuse_scratch"):
        assert name in hp and hasattr(pl._lib, name), name
    for name in ("fuse_points", "register_and_fuse", "release_fuse_scratch"):
        assert callable(getattr(pl.KinectFusion, name))


# ------------------------------------------------------------------------------------------------
# Accuracy on an analytic scene
def test_accuracy_on_an_analytic_scene():
    """A plane and a sphere at 48^3 seen from one origin, incidence up to 45 degrees, fused into an empty volume by the float32 model and by the same
    pipeline in float64: the distance of the fused field's zero crossing from the true surface along the rays.  The float32 model is held to twice
    the float64 pipeline's figure (rms and largest); the float64 pipeline itself is required to stay within half a voxel, which is the method's
    own error (projective distance, the mean over the rays through a voxel, trilinear interpolation) and not arithmetic.
    A crossing is found along 93.7 % of the rays; the others end at the rim of what was fused (the 45 degree cone, the sphere's shadow on the
    plane), where a corner of the interpolation cell was never visited: at least 90 % is required.
    Measured when this was written (voxel 62.5 mm): float64 rms 2.481 mm, largest 16.02 mm (0.26 voxel); float32 the same to six digits."""
    case, hits, dirs, cosi = fc.analytic_scene()
    assert len(hits) >= 20000 and cosi.min() >= np.cos(np.pi / 4) - 1e-12 and cosi.min() < 0.75
    hits, dirs = hits[:1500], dirs[:1500]                     # every ray is fused; the crossing is measured along the first 1500
    vs = float(case["vs"])
    err = {}
    for dtype in (np.float32, np.float64):
        value, weight = fc.fused_field(case, dtype)
        e = fc.crossing_error(case, value, weight, hits, dirs)
        assert np.isfinite(e).mean() >= 0.9, dtype
        e = e[np.isfinite(e)]
        err[dtype] = (float(np.sqrt((e * e).mean())), float(e.max()))
        print(dtype.__name__, "rays %d, zero crossing from the true surface: rms %.4g m, largest %.4g m (voxel %.4g m)" % (len(e), err[dtype][0], err[dtype][1], vs))
    assert err[np.float64][1] <= 0.5 * vs, "the float64 pipeline itself is not within half a voxel: a finding, not a tolerance"
    assert err[np.float32][0] <= 2 * err[np.float64][0] and err[np.float32][1] <= 2 * err[np.float64][1]
