"""GPU: the HIP kernels, through the C ABI, against the independently written float64 model and its central differences
(tests/independent_f64.py; no text shared with oracle/): kernel values to float32 rounding and — the point of the
product — the imaginary parts / h against finite-difference derivatives of a real-valued model, per kernel: integrate
voxel update, raycast vertex + normal, ICP rows + 27 sums, dual-complex residual (loss, gradient, second derivative; the full 6 x 6
Hessian from mixed seeds), six-pose Gauss-Newton sums (dense and band pass).
Measured figures are written to gpurun_out/independent_f64.json when that directory exists."""
import importlib
import json
import os

import numpy as np
import pytest

import independent_cases as ic

pytestmark = pytest.mark.gpu
CASES = [("s3", (2, 3), 0.0), ("s1", (0, 3), 0.05)]
LOG = {}


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    capi = importlib.import_module("x-slam_amd.capi")
    yield ic.GpuBackend(torch, capi, _m3_inverse)
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    if os.path.isdir(out) and LOG:
        json.dump(LOG, open(os.path.join(out, "independent_f64.json"), "w"), indent=1)


def _m3_inverse(R):
    """complex 3x3 inverse of an input transform (a test input, computed in float64 and rounded once)."""
    R = np.asarray(R, np.float64).reshape(3, 3, 2)
    inv = np.linalg.inv(R[..., 0] + 1j * R[..., 1])
    out = np.zeros((3, 3, 2), np.float32)
    out[..., 0], out[..., 1] = inv.real, inv.imag
    return out


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("scene,seed,threshold", CASES)
def test_integrate_values_and_derivatives(be, scene, seed, threshold, n):
    r = ic.check_integrate(be, n=n, scene=scene, seed=seed, threshold=threshold)
    LOG[f"integrate_{scene}_{n}"] = r
    assert r["n_band"] > 5000 and r["deriv_scale"] > 1.0
    assert r["written_disagree"] <= 1e-3
    assert r["value_bad"] <= 1e-3 and r["value_err_p999"] <= 2e-5
    assert r["deriv_bad"] <= 1e-3 and r["deriv_err_p999_rel"] <= 1e-4
    assert (r["bilinear_share"] > 0.9) == (threshold > 0)


@pytest.mark.parametrize("n", [128, 256])
@pytest.mark.parametrize("scene,seed,threshold", CASES)
def test_raycast_values_and_derivatives(be, scene, seed, threshold, n):
    r = ic.check_raycast(be, n=n, scene=scene, seed=seed, threshold=threshold)
    LOG[f"raycast_{scene}_{n}"] = r
    assert r["n_hit"] > 10000 and r["dvertex_scale"] > 1.0
    assert r["hit_disagree"] <= 2e-3 and r["normal_disagree"] <= 2e-3
    assert r["vertex_bad"] <= 2e-3 and r["vertex_err_p99"] <= 1e-5
    assert r["normal_bad"] <= 5e-3 and r["normal_err_p99"] <= 2e-4
    assert r["dvertex_bad"] <= 5e-3 and r["dvertex_err_p99_rel"] <= 2e-4
    assert r["dnormal_bad"] <= 5e-3 and r["dnormal_err_p99_rel"] <= 2e-4


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("scene,seed,threshold", CASES)
def test_icp_sums_and_derivatives(be, scene, seed, threshold, level):
    r = ic.check_icp(be, n=128, scene=scene, seed=seed, threshold=threshold, level=level)
    LOG[f"icp_{scene}_level{level}"] = r
    assert r["inliers"] > 0.5 * (480 >> level) * (640 >> level)
    assert abs(r["inliers"] - r["inliers_model"]) <= max(3, 5e-5 * r["inliers"])
    assert r["value_err_rel"] <= 2e-5 and r["deriv_err_rel"] <= 1e-4 and r["deriv_scale"] > 0


@pytest.mark.parametrize("scene,n", [("s3", 128), ("s1", 128), ("s3", 256)])
def test_hessian_loss_gradient_and_second_derivative(be, scene, n):
    r = ic.check_hessian(be, n=n, scene=scene)
    LOG[f"hessian_{scene}_{n}"] = r
    assert r["count"] > 1000 and abs(r["count"] - r["count_model"]) <= max(2, 1e-4 * r["count_model"])
    assert abs(r["loss"] - r["loss_model"]) <= 5e-4 * abs(r["loss_model"])
    # the gradient is a sum of terms of both signs (near a minimum they cancel: S1 at 128^3 has |grad| = 122 where the terms'
    # scale sqrt(loss * hessian) is 6 100): tolerance relative to the larger of the two
    assert abs(r["grad"] - r["grad_model"]) <= 5e-4 * max(abs(r["grad_model"]), (r["loss_model"] * abs(r["hess_model"])) ** 0.5)
    assert abs(r["hess"] - r["hess_model"]) <= 5e-4 * abs(r["hess_model"])


@pytest.mark.parametrize("n", [256, 512])
def test_survey_reference_kernel_figures_through_the_kernels(be, n):
    """The counts SURVEY.md section 6 recorded from the reference's own kernel bodies on scene S1 frame 0, through the HIP
    kernels alone (C ABI, no orchestrator): voxels written by integrate, rays hit by raycast, ICP inliers at level 0
    (tests/golden/survey_reference_kernel_figures.json; tolerances stated there)."""
    from helpers import intr_of, s1_transforms, synth
    fig = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "survey_reference_kernel_figures.json")))
    prm = synth.s1_params(n)
    T = s1_transforms(0, prm)
    d0 = synth.s1_frame(0)
    zero = (np.zeros(n ** 3, np.float32), np.zeros(n ** 3, np.int32), np.zeros(n ** 3, np.float32))
    state = be.integrate(zero, be.scale_depth(d0), prm, T, 0.0)
    U = int((state[1] != 0).sum())
    pv, pn, hits = be.raycast(state, prm, T)
    cv, cn = be.current_maps(d0, prm, 0)
    angle = float(np.sin(np.float32(15.0) / np.float32(180.0) * np.pi))
    _, inl = be.icp(T["Rc2w"], T["tc2w"], cv, cn, be.m3_inverse(T["Rc2w"]), T["tc2w"], intr_of(prm), pv, pn, 0.10, angle)
    LOG[f"survey_figures_{n}"] = dict(U=U, hits=hits, inliers=inl)
    assert abs(U - fig["integrate_U"][str(n)]) <= max(2, 1e-4 * fig["integrate_U"][str(n)])
    assert abs(hits - fig["raycast_hits"][str(n)]) <= 2
    assert abs(inl - fig["icp_inliers_level0"][str(n)]) <= 0.003 * fig["icp_inliers_level0"][str(n)]


# ---- the residual kernels with seeds along se(3) generators (tests/independent_cases.py: pair_pose, seeded_v2c) ----------------------
@pytest.mark.parametrize("scene,perturb,cross", [("s3", 3.0, (1, 3)), ("s1", 0.0, (3, 5))])
def test_full_hessian_from_21_launches(be, scene, perturb, cross):
    """xs_compute_local_tsdf_hessian seeded with eps1 along generator a and eps2 along b, for every pair a <= b (plus one pair with the
    eps1 eps2 input, which makes hessian / h^2 the exact entry of L(v2c exp(-theta_a G_a - theta_b G_b))): the 6 x 6 Hessian, each entry
    against the float64 model's four-point stencil.  S3 three units off the optimum, where the eps1 eps2 input's part of H_ab is 2.6e-3 of the
    scale; S1 at the frame's pose, where that part is below the tolerance (the entry is checked, the input is not exercised) — off the pose,
    one voxel on the sphere's depth edge moves S1's H_ab by more than the tolerance under the kernel's own float32 rounding."""
    r = ic.check_full_hessian(be, n=128, scene=scene, cross=(cross,), perturb=perturb)
    LOG[f"full_hessian_{scene}_128"] = dict(worst=r["worst"], count_diff=r["count_diff"], count_spread=r["count_spread"],
                                            entries={k: {f: e[f] for f in ("hess", "hess_model", "hess_err", "grad_err")} for k, e in r["entries"].items()})
    assert r["count_spread"] == 0 and len(r["entries"]) == 22
    for e in r["entries"].values():
        ic.assert_hessian_pair(e)


def _cropped_map(be, n, res):
    _, states = ic.two_frames(be, n, "s3", (0, 3), 0.0)
    return ic.crop(states[1][0], n, res)


@pytest.mark.parametrize("form", ["rows_not_16B", "slab", "address_4B"])
def test_hessian_pairs_on_the_other_scan_forms(be, form):
    """Mixed-seed pairs where the kernel scans otherwise than on the 16-byte aligned n^3 maps above: a 90 x 72 x 84 map
    (rows of 360 bytes: the one-column scan, a non-cubic volume), planes [40, 88) of the 128^3 map (z0 > 0, slab-relative addressing), and
    the 128^3 map at an address that is only 4-byte aligned (the one-column scan).  The eps1 eps2 pairs — on t for (t_y, omega_x), on R for
    (omega_x, omega_z) — are taken three units off the optimum (ic.perturbed_v2c), where that input's part of H_ab is 3.8e-4 .. 2.6e-3 and
    3.6e-3 .. 6.1e-3 of the scale: a scan that drops or misplaces it fails."""
    if form == "rows_not_16B":
        res = (90, 72, 84)
        kw = dict(n=96, gt=_cropped_map(be, 96, res), res=res)
    elif form == "slab":
        kw = dict(n=128, z0=40, z1=88)
    else:
        kw = dict(n=128, misalign=True)
    out = {}
    for a, b, cross in ((2, 4, False), (3, 5, False), (1, 3, True), (3, 5, True)):
        r = ic.check_hessian_pair(be, a, b, scene="s3", cross=cross, perturb=3.0 if cross else 0.0, **kw)
        out[f"{a}{b}{'x' if cross else ''}"] = r
        ic.assert_hessian_pair(r)
    LOG[f"hessian_pairs_{form}"] = out


@pytest.mark.parametrize("scene,n,z0,z1", [("s3", 128, 0, None), ("s1", 128, 0, None), ("s3", 256, 0, None), ("s3", 128, 40, 88)])
def test_gauss_newton_sums_against_the_model(be, scene, n, z0, z1):
    """xs_tsdf_gauss_newton_terms: all 29 sums (21 J^T J, 6 J^T r, sum r^2, count) against central differences of the float64 model's
    residual along each of the six seeded poses, over the whole map and over a slab."""
    r = ic.check_gn_terms(be, n=n, scene=scene, z0=z0, z1=z1)
    LOG[f"gn_terms_{scene}_{n}_{z0}_{n if z1 is None else z1}"] = r
    ic.assert_gn(r)


def test_band_pass_three_frames_against_the_model(be):
    """xs_tsdf_gauss_newton_terms_band, F = 3 frames in one launch, each with its own depth frame and its own perturbed pose: every
    frame's 29 sums against the model for that frame (a frame that read another frame's depth or poses fails)."""
    rs = ic.check_gn_band(be, n=128, scene="s3", frames=(1, 2, 3))
    LOG["gn_band_s3_128_F3"] = rs
    for r in rs:
        ic.assert_gn(r)


@pytest.mark.parametrize("scene", ["s3", "s1"])
def test_hessian_gradient_equals_gauss_newton_gradient(be, scene):
    """The Hessian kernel seeded with eps1 = h (-v2c G_k), eps2 = 0 and the six-pose kernel at the same real pose: grad / h ==
    2 sum d_k r / HSTEP for all six k, and the same voxel count."""
    r = ic.check_hessian_gn_identity(be, n=128, scene=scene)
    LOG[f"hessian_gn_identity_{scene}_128"] = r
    ic.assert_identity(r)
