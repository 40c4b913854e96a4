"""CPU-only: the float32 model of xs_render_views (tests/render_cases.py) against its float64 twin within the bound the cases file derives,
against the analytic ray-plane depth, the vacuity condition on the case set (so that the GPU comparison cannot pass on empty images), the
cull in the model, the host code of x-slam_amd/host/render_host.hpp under the sanitizers, and the new symbols of the ABI."""
import ctypes
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = rc.cases() + (rc.big_case(),)
DIFFERENT_CAP = 0.02      # the share of pixels whose crossing the two precisions may choose differently: a condition on the inputs


def test_vacuity_condition():
    """Across the case set the model alone produces every class and a hit without a normal, and hits are a quarter of all pixels: every image
    size, view count, step and min_weight the issue lists occurs."""
    counts = np.zeros(4, np.int64)
    nan_hits = pixels = 0
    for c in ALL:
        m = rc.expected(c["name"])
        counts += m["counts"].sum(axis=0).astype(np.int64)
        nan_hits += int(((m["cls"] == rc.HIT) & ~m["have"]).sum())
        pixels += m["cls"].size
        assert np.array_equal(m["counts"].sum(axis=1), np.full(len(c["R"]), c["rows"] * c["cols"]))       # the counts of a view sum to its pixels
    print("hit, backface, rejected, none:", counts, "hits without a normal:", nan_hits, "pixels:", pixels)
    assert (counts > 0).all() and nan_hits > 0
    assert counts.sum() == pixels and counts[0] * 4 >= pixels
    assert {(c["rows"], c["cols"]) for c in ALL} >= {(1, 1), (2, 3), (9, 17), (60, 80)}
    assert {len(c["R"]) for c in ALL} >= {1, 2, 3, 64}
    assert {round(float(c["step"] / c["vs"]), 3) for c in ALL} >= {1.0, 0.5, 2.5}
    assert {c["min_weight"] for c in ALL} == {1, 3}
    assert {c["shape"] for c in ALL} >= {(2, 2, 2), (3, 4, 5), (9, 5, 6), (33, 17, 20), (65, 33, 64)}
    assert any(c["pitch"] % 16 != 0 for c in ALL if c["shape"] == (33, 17, 20))
    # values of exactly 0 and -0 lie on a rendered surface
    v = next(c for c in ALL if c["name"] == "plane956_17x9")["vol"][0]
    bits = v.view(np.uint32)
    assert (bits == 0).any() and (bits == 0x80000000).any()


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_model_against_its_float64_twin(case):
    m, m64 = rc.expected(case["name"]), rc.expected(case["name"], f64=True)
    same = (m["cls"] == m64["cls"]) & (m["kh"] == m64["kh"])
    assert 1.0 - same.mean() <= DIFFERENT_CAP, 1.0 - same.mean()
    depth_bound, normal_bound = rc.bounds(case, m64)
    hit = same & (m["cls"] == rc.HIT)
    err = np.abs(m["depth"].astype(np.float64) - m64["depth"])
    both = hit & m["have"] & m64["have"]
    nerr = np.abs(m["normal"].astype(np.float64) - m64["normal"]).max(axis=1)
    if hit.any():
        print(case["name"], "depth: largest error %.3g, median bound %.3g;" % (err[hit].max(), np.median(depth_bound[hit])),
              "normal: largest error %.3g, median bound %.3g" % ((nerr[both].max(), np.median(normal_bound[both])) if both.any() else (0, 0)))
    assert (err[hit] <= depth_bound[hit]).all()
    assert (nerr[both] <= normal_bound[both]).all()
    # away from a hit both say "no depth", bit for bit
    assert not m["depth"][m["cls"] != rc.HIT].any() and not m["depth_u16"][m["cls"] != rc.HIT].any()
    assert np.array_equal(m["normal"].view(np.uint32)[np.broadcast_to(~m["have"][:, None], m["normal"].shape)] == rc.NAN_BITS, np.ones(3 * int((~m["have"]).sum()), bool))


def test_analytic_plane():
    """The stored field is the plane's distance over the truncation, linear in the whole volume: the trilinear value and the secant step are
    exact up to rounding, so the rendered depth is the ray-plane depth within the derived bound (the stored values' own float32 rounding, u
    vmax per corner, included)."""
    case, normal, offset, trunc = rc.analytic_plane()
    kw = dict(t_near=case["t_near"], t_far=case["t_far"], step=case["step"], min_weight=1)
    m = rc.render(case["vol"], case["vs"], case["R"], case["t"], case["intr"], case["rows"], case["cols"], **kw)
    m64 = rc.render(case["vol"], case["vs"], case["R"], case["t"], case["intr"], case["rows"], case["cols"], dtype=np.float64, **kw)
    hit = m["cls"] == rc.HIT
    assert hit.mean() > 0.3 and not (m["cls"] == rc.BACKFACE).any()
    d = m64["d"]
    tc = case["t"].astype(np.float64)[0]
    want = (offset - normal @ tc) / (normal[0] * d[0] + normal[1] * d[1] + normal[2] * d[2])
    depth_bound, _ = rc.bounds(case, m64)
    vmax = float(np.abs(case["vol"][0]).max())
    den = np.abs(m64["den"])
    extra = float(case["step"]) * 3 * rc.U * vmax / np.where(den > 0, den, np.inf)       # the corners' storage rounding moves F0 and F1 by u vmax each
    err = np.abs(m["depth"].astype(np.float64) - want)
    print("analytic plane: largest error %.3g m, median bound %.3g m" % (err[hit].max(), np.median((depth_bound + extra)[hit])))
    assert (err[hit] <= (depth_bound + extra)[hit]).all()
    # and the normal is the plane's
    both = hit & m["have"]
    n = m["normal"].astype(np.float64)
    assert both.mean() > 0.3
    assert np.abs(n[:, 0][both] - normal[0]).max() < 1e-4 and np.abs(n[:, 1][both] - normal[1]).max() < 1e-4 and np.abs(n[:, 2][both] - normal[2]).max() < 1e-4


@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_cull_changes_nothing_in_the_model(case):
    a, b = rc.expected(case["name"]), rc.expected(case["name"], cull=True)
    for k in rc.OUTPUTS + ("cls", "kh"):
        assert rc.same_output(k, a[k], b[k]), k
    assert b["reads"] <= a["reads"]


def test_the_cull_skips_reads_somewhere():
    assert any(rc.expected(c["name"], cull=True)["reads"] < 0.7 * rc.expected(c["name"])["reads"] for c in ALL)


def test_mask_words():
    """The mask's layout on a volume wider than one word of bricks: bit bx & 31 of word (bz BY + by) WX + (bx >> 5)."""
    value = np.ones((9, 8, 300), np.float32)
    weight = np.ones((9, 8, 300), np.int32)
    value[8, 3, 299] = -1.0          # brick (37, 0, 1)
    value[0, 0, 0] = -1.0            # brick (0, 0, 0), below min_weight 2
    value[2, 7, 255] = -0.5          # brick (31, 0, 0)
    weight[2, 7, 255] = 2
    weight[8, 3, 299] = 5
    value[4, 4, 100] = -0.0          # not below zero
    w1, w2 = rc.mask_words((value, weight), 1), rc.mask_words((value, weight), 2)
    assert rc.mask_dims((300, 8, 9)) == (38, 1, 2, 2)
    assert w1.tolist() == [0x80000001, 0, 0, 1 << 5] and w2.tolist() == [0x80000000, 0, 0, 1 << 5]
    assert rc.workspace_bytes((512, 512, 512)) == 256 + 3072 + 32768


def test_render_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/render_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/render_selftest.cpp): the
    validation table, the mask sizes and the pose conversion; then its sample count against the float32 model's on the cases' ranges."""
    exe = str(tmp_path / "render_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "x-slam_amd", "host"), os.path.join(ROOT, "tests", "cxx", "render_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    ranges = [(c["t_near"], c["t_far"], c["step"]) for c in ALL] + [(0.2, 5.0, 0.05), (0.2, 5.0, 0.01), (0.0, 4096.5, 1.0), (0.1, 0.1000001, 1e-9)]
    for t_near, t_far, step in ranges:
        r = subprocess.run([exe, "samples", repr(float(np.float32(t_near))), repr(float(np.float32(t_far))), repr(float(np.float32(step)))], capture_output=True,
                           text=True, timeout=60, env=env)
        assert r.returncode == 0 and int(r.stdout) == rc.samples(t_near, t_far, step), (t_near, t_far, step, r.stdout)


def test_abi_exports_and_declares_the_render_calls():
    low = ("xs_render_workspace_bytes", "xs_render_mask_build", "xs_render_views")
    high = ("xs_kf_render_views", "xs_kf_render_volume", "xs_kf_render_map", "xs_kf_render_checkpoint")
    hip = ctypes.CDLL(os.path.join(ROOT, "x-slam_amd", "libxslam_hip.so"), mode=ctypes.RTLD_GLOBAL)
    host = ctypes.CDLL(os.path.join(ROOT, "x-slam_amd", "libxslam_host.so"))
    for lib, names, header in ((hip, low, "xslam_amd.h"), (host, high, "xslam_amd_pipeline.h")):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        for n in names:
            assert hasattr(lib, n), n
            assert re.search(r"\b%s\s*\(" % n, text), n
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    assert set(low) <= set(capi._SIGS) and set(high) <= set(pl._SIGS)
    assert capi.abi_version() == 3                                   # additive
    assert ctypes.sizeof(capi.RenderOpts) == 28 and capi.RENDER_MAX_VIEWS == rc.MAX_VIEWS == 64
    for res in ((512, 512, 512), (33, 17, 20), (1, 1, 1), (300, 8, 9)):
        assert capi.render_workspace_bytes(res) == rc.workspace_bytes(res)
    assert capi.render_workspace_bytes((0, 8, 8)) == 0 and capi.render_workspace_bytes((8, 8, 300000)) == 0
    assert all(hasattr(pl.KinectFusion, n) for n in ("render_views", "render_map", "render_checkpoint")) and hasattr(pl, "save_view_pgm")
    assert pl.RenderedViews._fields == ("depth", "depth_u16", "normal", "shade", "counts")
