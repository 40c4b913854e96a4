"""CPU-only: the model xs_tsdf_register_terms is held to (tests/register_cases.py): the conditions on its cases, the mutants the cases must tell
apart, the model against its float64 twin within the derived bound, J against central differences of the twin on the linear field, the host
algebra of x-slam_amd/host/register_host.hpp through the exported functions and under the sanitizers, a registration loop of the model and of
the twin on an analytic sphere, and the bindings of every layer."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import align_cases as ac
import merge_cases as mc
import register_cases as rg
import sample_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = rg.cases() + (rg.big_case(),)
F32 = np.float32
LOOP_AGREEMENT_M = rg.LOOP_AGREEMENT_M     # measured by test_twin_loop below, stated with its factor 4 in register_cases.py


@pytest.fixture(scope="module")
def pl():
    return importlib.import_module("x-slam_amd.pipeline")


def test_the_case_set_is_the_issues():
    names = [c["name"] for c in ALL]
    assert len(set(names)) == len(names)
    assert {c["shape"] for c in ALL} == {(2, 2, 2), (3, 4, 5), (33, 17, 20), (65, 33, 64)}
    assert {1, 5, 6, 63, 64, 65, 255, 257, rg.BIG_N} <= {c["n"] for c in ALL}
    assert {c["min_weight"] for c in ALL} == {1, 3} and {c["max_residual"] for c in ALL} == {float(F32(0.9)), float(F32(0.3))}
    assert any((c["xform"] == sc.IDENTITY12).all() for c in ALL) and any((c["xform"] != sc.IDENTITY12).any() for c in ALL)
    assert any(c["pitch"] > c["shape"][0] * 4 and c["offset"] for c in ALL)
    big = next(c for c in ALL if c["n"] == rg.BIG_N)
    assert rg.nblocks_of(big["n"]) == 4096 and (big["n"] + 63) // 64 > 4 * 4096 and len(rg.all_points(big)) == rg.BIG_N


@pytest.mark.parametrize("case", ALL, ids=lambda c: c["name"])
def test_conditions(case):
    """n >= 255: every gate drops a point and a point is kept.  Every case: no |r| within 2^-22 of max_residual unless equal to it; every kept
    point is OK with a gradient in the twin too; where values of exactly +-max_residual are planted, the points on them are kept."""
    m = rg.expected(case["name"])["point"]
    drops, kept, near = rg._conditions(case, m)
    print(case["name"], "dropped by status, gradient, residual:", drops, "kept:", kept)
    assert near == 0
    assert sum(drops) + kept == len(case["base_pts"])
    if case["n"] >= 255:
        assert min(drops) > 0 and kept > 0, (drops, kept)
    m64 = rg.point_terms(case, np.float64, keep=m["kept"])
    assert (m64["ok"] & m64["gok"])[m["kept"]].all()
    if case["planted"] is not None:
        on = np.abs(m["r"]) == F32(case["max_residual"])
        assert on.sum() >= len(case["planted"]) and m["kept"][on].all()
    assert rg.expected(case["name"])["sums"][28] == kept * case["tile"]
    if case["name"] == "big_rows":
        assert rg.high_rows_kept(case, m).sum() >= 50


def test_chunk_order_and_fsum_agree():
    """The kernel-ordered sums against math.fsum: within the tolerance the GPU test grants the kernel; the count equal."""
    for case in ALL:
        e = rg.expected(case["name"])
        assert e["sums"][28] == e["fsum"][28]
        assert (np.abs(e["sums"] - e["fsum"]) <= e["tolerance"]).all(), case["name"]


@pytest.mark.parametrize("mutant", rg.MUTANTS)
def test_every_mutant_changes_a_sum(mutant):
    """Each mistake moves a sum of some case beyond the tolerance of the GPU comparison (or changes the count)."""
    hit = []
    for case in (rg.wrap_case(),) if mutant == "row_wrap32" else ALL:
        good = rg.expected(case["name"]) if mutant != "row_wrap32" else dict(sums=rg.evaluate(case)["sums"], tolerance=rg.tolerance(rg.evaluate(case)["terms"]))
        bad = rg.evaluate(case, mutant=mutant)
        d = np.abs(bad["sums"] - good["sums"])
        if (d > good["tolerance"]).any():
            hit.append(case["name"])
    print(mutant, "changes", hit)
    assert hit, mutant
    if mutant == "row_wrap32":     # and the unwrapped model is unmoved by the pitch
        plain = next(c for c in ALL if c["name"] == "v345_n63_rigid")
        assert np.array_equal(rg.evaluate(rg.wrap_case())["sums"], rg.expected(plain["name"])["sums"])


@pytest.mark.parametrize("case", ALL, ids=lambda c: c["name"])
def test_model_agrees_with_its_float64_twin(case):
    """Each of the 28 sums over the base points within the derived bound of the twin's; the counts equal."""
    m32 = rg.expected(case["name"])["point"]
    m64 = rg.point_terms(case, np.float64, keep=m32["kept"])
    s32, s64 = rg.chunk_sums(rg.terms29(m32)), rg.chunk_sums(rg.terms29(m64))
    b = rg.bound(case, m32, m64)
    assert s32[28] == s64[28] == m32["kept"].sum()
    assert np.isfinite(s32).all() and np.isfinite(s64).all() and np.isfinite(b).all()
    d = np.abs(s32 - s64)
    print(case["name"], "largest |model - twin| / bound: %.3g" % float((d[:28] / np.maximum(b[:28], 1e-300)).max()))
    assert (d[:28] <= b[:28]).all(), d / np.maximum(b, 1e-300)
    # the bound says something: it is small against the sums it bounds wherever a point is kept
    if m32["kept"].sum() > 50:
        assert b[27] < 1e-3 * max(s64[27], 1e-30)


def test_jacobian_is_the_derivative_on_the_linear_field():
    """J of the float32 model against central differences of the float64 twin's F(exp(eps e_k) T p) on the linear field, identity and rigid.  The
    interpolant of a linear field is that field, whose derivative along generator k is a_k (translations) and (P x a)_k (rotations) exactly;
    the model's gradient and the twin's interpolant are each within sample_cases' gradient bound for the linear case (storage = 1) of that
    slope, the cross product adds the error of P and three roundings, and the difference quotient eps^2 |P| |a| of curvature."""
    (value, weight), field = sc.linear_volume(sc.LINEAR_SHAPE, sc.VS2, sc.LINEAR_A, sc.LINEAR_B)
    vol = (value, weight)
    base = sc.random_points(sc.LINEAR_SHAPE, sc.VS2, 300, 71, margin=-1.0)
    a = np.array(sc.LINEAR_A)
    eps = 1e-4
    for rigid_seed in (None, 31):
        x12, T = (sc.IDENTITY12.copy(), np.eye(4)) if rigid_seed is None else sc.rigid(rigid_seed, 0.5, (0.1, -0.05, 0.07))
        pts = sc.points_for(x12, T, base)
        case = dict(kind="points", vol=vol, vs=sc.VS2, pts=pts, base_pts=pts, xform=x12, min_weight=1, grad=None, max_residual=100.0, pitch=sc.LINEAR_SHAPE[0] * 4)
        m = rg.point_terms(case)
        assert m["kept"].all()
        L = max(float(np.abs(m["P"][c]).max()) for c in range(3))
        Ep = rg._ep_of(case)
        _, _, bg = sc.bounds_from(Ep, L, sc.VS2, field, storage=1.0)
        p64 = np.concatenate([pts.astype(np.float64), np.ones((len(pts), 1))], axis=1)
        x64 = np.concatenate([x12[:9].astype(np.float64).reshape(3, 3), x12[9:].astype(np.float64).reshape(3, 1)], axis=1)
        P64 = p64 @ np.vstack([x64, [0, 0, 0, 1]]).T
        worst = np.zeros(6)
        for k in range(6):
            d = np.zeros(6)
            F = []
            for sign in (1.0, -1.0):
                d[k] = sign * eps
                Q = (P64 @ ac.se3_exp(d).T)[:, :3]
                st, out = sc.trilinear([value.astype(np.float64)], weight, np.float64(sc.VS2), 1, [Q[:, c] for c in range(3)], np.float64)
                assert (st == sc.OK).all()
                F.append(out[0])
            cd = (F[0] - F[1]) / (2 * eps)
            bound_k = 2 * bg + 1e-9 if k < 3 else 2 * (2 * L * bg) + 2 * np.abs(a).max() * Ep + 6 * sc.U * L * np.abs(a).max() + eps * eps * L * np.abs(a).max() + 1e-9
            err = np.abs(m["J"][k].astype(np.float64) - cd)
            worst[k] = err.max() / bound_k
            assert (err <= bound_k).all(), (rigid_seed, k, err.max(), bound_k)
            assert bound_k < 1e-3     # against slopes of 0.6 .. 1.3
        print("rigid" if rigid_seed else "identity", "largest |J - central difference| / bound per generator:", np.round(worst, 3))


def test_register_step_against_numpy(pl):
    """xs_host_register_step against the float64 restatement on the sums of J = (g, P x g) problems, unscaled: the step that solves a linear
    problem exactly recovers its twist; fewer than six points and an indefinite system refuse and leave T alone; it is align_step's algebra."""
    rng = np.random.default_rng(61)
    for it in range(60):
        g = rng.normal(size=(50, 3)) * 10.0 ** rng.uniform(-1, 1)
        P = rng.uniform(-2, 2, size=(50, 3))
        J = np.concatenate([g, np.cross(P, g)], axis=1)
        twist = rng.normal(size=6) * 10.0 ** rng.uniform(-6, -1)
        r = -J @ twist
        s = np.zeros(29)
        s[:21] = (J.T @ J)[np.triu_indices(6)]
        s[21:27], s[27], s[28] = J.T @ r, r @ r, 50
        T = np.eye(4)
        T[:3, :3] = mc.rotation(rng.normal(size=3), rng.uniform(-3, 3))
        T[:3, 3] = rng.uniform(-5, 5, 3)
        damping = [0.0, 1e-3, 0.5][it % 3]
        taken, got = pl.register_step(s, damping, T)
        ok, want = ac.step(s, damping, T)
        assert taken and ok
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), it
        assert np.array_equal(got, pl.align_step(s, damping, T)[1])
        if damping == 0.0:
            assert np.abs(got - ac.se3_exp(twist) @ T).max() <= 1e-9 * max(1.0, np.abs(T).max())
    few = s.copy()
    few[28] = 5
    taken, got = pl.register_step(few, 1e-3, T)
    assert not taken and np.array_equal(got, T)
    bad = s.copy()
    bad[0] = -1.0
    taken, got = pl.register_step(bad, 1e-3, T)
    assert not taken and np.array_equal(got, T)


def test_twin_loop():
    """An analytic sphere at 24^3, points on its surface plus 20 % far outliers, the start 1.5 voxels and 2 degrees off: the model's loop and the
    twin's loop both end with a loss below the one they started at, and agree on T within LOOP_AGREEMENT_M at every corner of the volume."""
    case, pts, T_true, T0 = rg.loop_scene()
    n, vs = case["shape"][0], float(case["vs"])
    start = ac.corner_displacement(T0, T_true, (n, n, n), vs)
    c = 0.5 * n * vs * np.ones(3)
    D = T0 @ np.linalg.inv(T_true)
    assert 1.4 * vs < np.linalg.norm(D[:3, :3] @ c + D[:3, 3] - c) < 1.6 * vs
    assert abs(np.degrees(np.arccos((np.trace(D[:3, :3]) - 1) / 2)) - 2.0) < 1e-6
    ends = []
    for twin in (False, True):
        ok, T, hist, s = rg.loop(case, pts, T0, 10, twin=twin)
        assert ok and len(hist) == 11 and np.isfinite(T).all()
        end = ac.corner_displacement(T, T_true, (n, n, n), vs)
        E = T @ np.linalg.inv(T_true)
        print("twin" if twin else "model", "corner distance from T_true: start %.4g m, end %.4g m (%.3g voxels); the sphere's centre: start %.4g m, end %.4g m; "
              "kept %d of %d; loss history %s" % (start, end, end / vs, np.linalg.norm(D[:3, :3] @ c + D[:3, 3] - c), np.linalg.norm(E[:3, :3] @ c + E[:3, 3] - c),
                                                  int(s[28]), len(pts), np.array2string(hist, precision=5)))
        assert hist[-1] < hist[0]
        ends.append(T)
    apart = ac.corner_displacement(ends[0], ends[1], (n, n, n), vs)
    print("model loop and twin loop end %.3g m apart (bound %.3g)" % (apart, LOOP_AGREEMENT_M))
    assert apart <= LOOP_AGREEMENT_M


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/register_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/register_selftest.cpp)."""
    exe = str(tmp_path / "register_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "x-slam_amd", "host"), os.path.join(ROOT, "tests", "cxx", "register_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_sizes_and_bindings(pl):
    """Tickets and 4096 records of 32 doubles per transform; 0 outside 1 .. 32; the entry points of every layer, in headers, libraries and tables."""
    capi = importlib.import_module("x-slam_amd.capi")
    for n in (1, 5, 32):
        assert capi.register_workspace_bytes(n) == 256 + n * 4096 * 32 * 8
    for n in (0, -1, 33):
        assert capi.register_workspace_bytes(n) == 0
    text = {h: open(os.path.join(ROOT, "include", h)).read() for h in ("xslam_amd.h", "xslam_amd_pipeline.h")}
    for n in ("xs_tsdf_register_terms", "xs_tsdf_register_workspace_bytes"):
        assert n in capi._SIGS and hasattr(capi._lib, n) and n + "(" in text["xslam_amd.h"], n
    for n in ("xs_kf_register_points", "xs_kf_register_map", "xs_kf_register_checkpoint", "xs_host_register_step"):
        assert n in pl._SIGS and hasattr(pl._lib, n) and n + "(" in text["xslam_amd_pipeline.h"], n
    assert "#define XS_REGISTER_MAX_TRANSFORMS 32" in text["xslam_amd.h"]
    assert capi.REGISTER_MAX_TRANSFORMS == 32 and capi.abi_version() == 3
    for name in ("register_points", "register_map_points", "register_checkpoint_points"):
        assert callable(getattr(pl.KinectFusion, name))
    assert "truncated field" in pl.KinectFusion.register_points.__doc__ and "0.9" in pl.KinectFusion.register_points.__doc__
    assert callable(pl.register_step) and callable(capi.register_terms)
