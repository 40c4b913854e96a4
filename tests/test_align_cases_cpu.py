"""CPU-only: the model the map alignment is held to (tests/align_cases.py) against its float64 twin within the derived bound, the conditions
on its cases, the host algebra of x-slam_amd/host/align_host.hpp through the exported functions and under the sanitizers, a twin loop that
ends at the truth, and the bindings of every layer."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import align_cases as ac
import merge_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [((9, 10, 13), 257, False), ((9, 10, 13), 0, True), ((70, 33, 5), 255, False), ((70, 33, 5), 0, True), ((3, 2, 2), 257, False), ((2, 2, 2), 255, False)]


@pytest.fixture(scope="module")
def pl():
    return importlib.import_module("x-slam_amd.pipeline")


@pytest.mark.parametrize("sshape,count,built", CASES)
def test_model_agrees_with_its_float64_twin(pl, sshape, count, built):
    """Every map, both min_weights: each of the 28 sums within its derived bound of the twin's, the counts equal, no entry near the
    residual threshold; and the case is what the module says it is: over its maps every gate drops entries and entries are kept.  The
    model's seed step and its maps built from a transform are the library's."""
    assert pl.align_seeded_maps(np.eye(4), 1.0, 1.0)[0, 9, 1] == np.float32(ac.H)
    assert np.array_equal(ac.case_maps(sshape)["ratio_2"].view(np.uint32), pl.align_seeded_maps(np.eye(4), 2 * 0.0625, 0.0625).view(np.uint32))
    drops = np.zeros(3, np.int64)
    kept = 0
    for name in ac.case_maps(sshape):
        for mw in ac.MIN_WEIGHTS:
            ev = ac.expected(sshape, count, built, name, mw)
            assert ev["near_threshold"] == 0, (name, mw)
            assert ev["sums32"][28] == ev["sums64"][28] == ev["kept"].sum()
            d = np.abs(ev["sums32"] - ev["sums64"])
            assert (d[:28] <= ev["bound"][:28]).all(), (name, mw, d / np.maximum(ev["bound"], 1e-300))
            assert np.isfinite(ev["sums32"]).all() and np.isfinite(ev["bound"]).all()
            drops += (ev["outside"], ev["weight"], ev["residual"])
            kept += int(ev["kept"].sum())
            n = len(ev["kept"])
            assert ev["outside"] + ev["weight"] + ev["residual"] + ev["kept"].sum() == n
            if name == "miss":
                assert ev["outside"] == n and not ev["sums32"].any()
            if name == "far_face" and n:
                xyz = ac.case(sshape, count, built)[0]
                last = (xyz == np.array(ac.dst_shape_of(sshape)) - 1).any(axis=1)
                assert not ev["kept"][last].any()
    assert (drops > 0).all() and kept > 0, (drops, kept)
    if min(sshape) > 3:
        assert kept > 50, (drops, kept)


def test_seeded_maps(pl):
    """align_seeded_maps: real parts merge_affine's bit for bit for every seed; the whole result the numpy restatement's; imaginary parts / h
    the central differences of merge_affine along each generator in float64 to 1e-6 relative; merge_affine's refusals."""
    rng = np.random.default_rng(53)
    gens = []
    for k in range(6):
        G = np.zeros((4, 4))
        if k < 3:
            G[k, 3] = 1.0
        else:
            a = k - 3
            b, c = (a + 1) % 3, (a + 2) % 3
            G[c, b], G[b, c] = 1.0, -1.0
        gens.append(G)

    def affine_f64(T, vd, vs):     # merge_affine without the final rounding
        m = np.zeros(12)
        for a in range(3):
            m[3 * a:3 * a + 3] = T[a, :3] * vd / vs
            m[9 + a] = (T[a, :3].sum() * 0.5 * vd + T[a, 3]) / vs - 0.5
        return m

    for it in range(40):
        T = np.eye(4)
        if it:
            T[:3, :3] = mc.rotation(rng.normal(size=3), rng.uniform(-3, 3))
            T[:3, 3] = rng.uniform(-5, 5, 3)
        for vd, vs in ((0.1, 0.1), (0.25, 0.125), (0.05, 0.1), (float(np.float32(0.03)), 0.07)):
            got = pl.align_seeded_maps(T, vd, vs)
            assert got.shape == (6, 12, 2) and got.dtype == np.float32
            want_re = pl.merge_affine(T, vd, vs)
            for k in range(6):
                assert mc.same_bits(got[k, :, 0], want_re), (it, k)
            assert np.array_equal(got.view(np.uint32), ac.seeded_maps(T, vd, vs).view(np.uint32))
            eps = 1e-6
            for k in range(6):
                cd = (affine_f64((np.eye(4) + eps * gens[k]) @ T, vd, vs) - affine_f64((np.eye(4) - eps * gens[k]) @ T, vd, vs)) / (2 * eps)
                d = got[k, :, 1].astype(np.float64) / ac.H
                assert np.abs(d - cd).max() <= 1e-6 * max(np.abs(cd).max(), 1e-30), (it, k)
    # -0 care: a zero real part keeps its sign under the seed
    Tz = np.eye(4)
    Tz[0, 1] = -0.0
    assert np.signbit(pl.align_seeded_maps(Tz, 0.1, 0.1)[:, 1, 0]).all()
    for bad in (np.full((4, 4), np.nan), np.diag([1, 1, np.inf, 1])):
        with pytest.raises(ValueError):
            pl.align_seeded_maps(bad, 0.1, 0.1)
    for vd, vs in ((0.0, 0.1), (0.1, 0.0), (-0.1, 0.1), (np.inf, 0.1)):
        with pytest.raises(ValueError):
            pl.align_seeded_maps(np.eye(4), vd, vs)


def test_align_step_against_numpy(pl):
    """xs_host_align_step against the float64 restatement (Cholesky through numpy, Rodrigues with the small-angle branch): steps of every
    size from 1e-9 to 1 rad; fewer than six voxels and an indefinite system refuse and leave T alone."""
    rng = np.random.default_rng(59)
    for it in range(60):
        J = rng.normal(size=(40, 6)) * 10.0 ** rng.uniform(-1, 2, 6)
        r = rng.normal(size=40) * 10.0 ** rng.uniform(-9, 0)
        s = np.zeros(29)
        A = J.T @ J
        s[:21] = A[np.triu_indices(6)]
        s[21:27], s[27], s[28] = J.T @ r, r @ r, 40
        T = np.eye(4)
        T[:3, :3] = mc.rotation(rng.normal(size=3), rng.uniform(-3, 3))
        T[:3, 3] = rng.uniform(-5, 5, 3)
        damping = [0.0, 1e-3, 0.5][it % 3]
        taken, got = pl.align_step(s, damping, T)
        ok, want = ac.step(s, damping, T)
        assert taken and ok
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), it
        assert np.array_equal(got[3], [0, 0, 0, 1])
        R = got[:3, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    few = s.copy()
    few[28] = 5
    taken, got = pl.align_step(few, 1e-3, T)
    assert not taken and np.array_equal(got, T) and not ac.step(few, 1e-3, T)[0]
    bad = s.copy()
    bad[0] = -1.0
    taken, got = pl.align_step(bad, 1e-3, T)
    assert not taken and np.array_equal(got, T) and not ac.step(bad, 1e-3, T)[0]


def test_twin_loop_ends_at_the_truth(pl):
    """The exact whole-voxel shift of a sphere's TSDF at 24^3 from a start half a voxel and 0.5 degrees off: the twin's loop and the model's
    both end with a loss below 1e-4 of the loss they started at, the losses never rise, and both end within a hundredth of a voxel edge
    of the truth at every corner of the volume."""
    n, vs = 24, 0.05
    this, other, T_true = ac.sphere_scene(n, voxel_size=vs)
    xyz, gt = ac.band_of(this)
    assert len(gt) > 1000
    at_truth = ac.evaluate(xyz, gt, other, ac.seeded_maps(T_true, vs, vs))
    assert at_truth["sums32"][27] == 0.0 and at_truth["sums64"][27] == 0.0 and at_truth["sums32"][28] > 1000
    T0 = ac.perturbed(T_true, (n, n, n), vs)
    assert 0.4 * vs < np.linalg.norm((T0 @ np.linalg.inv(T_true))[:3, 3] - (np.eye(3) - (T0 @ np.linalg.inv(T_true))[:3, :3]) @ (0.5 * n * vs * np.ones(3))) < 0.6 * vs
    ends = []
    for twin in (True, False):
        ok, T, hist, ev = ac.loop(xyz, gt, other, T0, vs, vs, 10, twin=twin)
        assert ok and len(hist) == 11
        # the library's step on the last pass's sums is the restatement's
        s_last = ac.scale_sums(ev["sums64" if twin else "sums32"])
        lib, mine = pl.align_step(s_last, 1e-3, T), ac.step(s_last, 1e-3, T)
        assert lib[0] and mine[0] and np.abs(lib[1] - mine[1]).max() <= 1e-12
        assert hist[-1] < 1e-4 * hist[0], (twin, hist)
        assert (np.diff(hist) <= 1e-12 * hist[0]).all(), (twin, hist)
        assert ac.corner_displacement(T, T_true, (n, n, n), vs) < 0.01 * vs
        ends.append(T)
    assert ac.corner_displacement(ends[0], ends[1], (n, n, n), vs) < 1e-4 * vs


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/align_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/align_selftest.cpp)."""
    exe = str(tmp_path / "align_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "x-slam_amd", "host"), os.path.join(ROOT, "tests", "cxx", "align_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_sizes_and_bindings(pl):
    """Tickets, 32 x 144 floats of maps and 4096 records of 32 doubles per transform; 0 outside 1 .. 32; the entry points of every layer."""
    capi = importlib.import_module("x-slam_amd.capi")
    sh = importlib.import_module("x-slam_amd.sharded")
    for n in (1, 5, 32):
        assert capi.tsdf_align_workspace_bytes(n) == 256 + 32 * 144 * 4 + n * 4096 * 32 * 8
    for n in (0, -1, 33):
        assert capi.tsdf_align_workspace_bytes(n) == 0
    for n in ("xs_tsdf_align_terms", "xs_tsdf_align_workspace_bytes"):
        assert n in capi._SIGS and hasattr(capi._lib, n), n
    for n in ("xs_kf_align_map", "xs_kf_align_checkpoint", "xs_host_align_seeded_maps", "xs_host_align_step"):
        assert n in pl._SIGS and hasattr(pl._lib, n), n
    assert capi.ALIGN_MAX_TRANSFORMS == 32 and capi.abi_version() == 3
    for cls in (pl.KinectFusion, sh.ShardedKinectFusion):
        assert callable(cls.align_map) and callable(cls.align_checkpoint)
        assert "merge_map(other, kf.align_map(other, T_guess)[1])" in cls.align_map.__doc__
    assert callable(pl.align_seeded_maps) and callable(pl.align_step) and callable(capi.tsdf_align_terms) and callable(capi.align_seeded_maps)
