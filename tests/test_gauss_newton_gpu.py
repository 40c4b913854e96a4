"""GPU: first-order CSFD Gauss-Newton terms of the TSDF residual (xs_tsdf_gauss_newton_terms, BASELINE config 5)
against the oracle, their consistency with the dual-complex Hessian kernel, and the pose refinement loop built on
them (RelocalizeGaussNewton)."""
import importlib

import numpy as np
import pytest

from helpers import intr_of, s1_transforms, synth, tranc_dist
from independent_cases import HSTEP, seeded_poses

W, H = synth.WIDTH, synth.HEIGHT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import Oracle
    return Oracle()


def twist_matrix(xi):
    """se3Exp for a small real twist (v, omega), double precision (test-side reference)."""
    v, w = np.asarray(xi[:3], float), np.asarray(xi[3:], float)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        R, V = np.eye(3) + K, np.eye(3) + K
    else:
        R = np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * K + (th - np.sin(th)) / th ** 3 * K @ K
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = V @ v
    return T


def test_gn_terms_equal_oracle(dev, oracle):
    torch, capi, _ = dev
    n = 64
    prm = synth.s1_params(n)
    res = [n, n, n]
    v, w, g = oracle.new_volume(res)
    for k in (0, 1, 2):
        T = s1_transforms(k, prm)
        oracle.integrate(oracle.scale_depth(synth.s1_frame(k)), v, w, g, res, tranc_dist(prm), 100, T["Rv2c"], T["tv2c"], intr_of(prm),
                         prm["tsdf_voxel_size"])
    T3 = s1_transforms(3, prm)
    v2c = np.eye(4); v2c[:3, :3] = np.asarray(T3["Rv2c"])[..., 0]; v2c[:3, 3] = np.asarray(T3["tv2c"])[..., 0]
    Rs, ts = seeded_poses(np.linalg.inv(v2c))
    ds = oracle.scale_depth(synth.s1_frame(3))
    want = oracle.tsdf_gn_terms(ds, res, prm["tsdf_voxel_size"], Rs, ts, tranc_dist(prm), intr_of(prm), v)
    assert want[28] > 1000 and want[27] > 0
    ws = torch.zeros(capi.tsdf_reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    out = torch.zeros(32, dtype=torch.float64, device="cuda")
    gt = torch.from_numpy(v).cuda()
    capi.tsdf_gauss_newton_terms(torch.from_numpy(ds).cuda(), W * 4, H, W, intr_of(prm), res, prm["tsdf_voxel_size"], Rs, ts, tranc_dist(prm),
                                 gt, ws, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:29]
    assert got[28] == want[28]
    assert np.allclose(got[27], want[27], rtol=1e-9)
    # CSFD derivative sums: 1e-6 relative to the largest entry of each group (north_star's derivative tolerance)
    assert np.all(np.abs(got[:21] - want[:21]) <= 1e-6 * np.abs(want[:21]).max())
    assert np.all(np.abs(got[21:27] - want[21:27]) <= 1e-6 * np.abs(want[21:27]).max())
    # slab split adds up (what the sharded ranks all-reduce)
    parts = np.zeros(29)
    for z0, z1 in ((0, 20), (20, 45), (45, n)):
        out.zero_()
        capi.tsdf_gauss_newton_terms(torch.from_numpy(ds).cuda(), W * 4, H, W, intr_of(prm), res, prm["tsdf_voxel_size"], Rs, ts,
                                     tranc_dist(prm), gt[z0 * n * n:], ws, out, z0=z0, z1=z1)
        torch.cuda.synchronize()
        parts += out.cpu().numpy()[:29]
    assert parts[28] == got[28] and np.allclose(parts[:28], got[:28], rtol=1e-10, atol=1e-12 * np.abs(got[:28]).max())
    # the gradient agrees with finite differences of the real-valued loss kernel along each generator
    base = np.linalg.inv(v2c)
    eps = 2e-4
    for k in (0, 2, 4):
        vals = []
        for sgn in (+1, -1):
            xi = np.zeros(6); xi[k] = sgn * eps
            m = np.linalg.inv(twist_matrix(xi) @ base)
            o2 = torch.zeros(2, dtype=torch.float64, device="cuda")
            capi.compute_local_tsdf_loss(torch.from_numpy(ds).cuda(), W * 4, H, W, intr_of(prm), res, prm["tsdf_voxel_size"],
                                         m[:3, :3].astype(np.float32), m[:3, 3].astype(np.float32), tranc_dist(prm), gt, ws, o2)
            torch.cuda.synchronize()
            vals.append(o2.cpu().numpy().copy())
        if vals[0][1] == vals[1][1] == got[28]:   # same voxel set: the loss is smooth between the two
            fd = (vals[0][0] - vals[1][0]) / (2 * eps)
            csfd = 2.0 * got[21 + k] / float(HSTEP)
            assert abs(fd - csfd) <= 0.05 * max(abs(csfd), 1e-3 * np.abs(got[21:27]).max() * 2 / float(HSTEP))


def test_posted_launch_publishes_one_record_whatever_happens(dev, oracle):
    """xs_tsdf_gauss_newton_terms_ex through the C ABI: a launch enqueued before its poses exist takes them from the mailbox and publishes the same
    29 sums, bit for bit, as the launch that got them as arguments; a launch that is told to leave, and one whose poses never come, publish the
    sequence word with bit 63 set, sum nothing, and leave the workspace's arrival ticket at zero (every workgroup arrives, whatever it did: a launch
    some of whose workgroups saw poses and others not could otherwise never finish, and would leave a ticket the next launch trips over) — the next
    launch on the same workspace is unaffected.  At 512^3, where not every workgroup is resident at once, the workgroups that start after one
    has given up do not wait their own second out."""
    import time
    torch, capi, _ = dev
    n = 64
    prm = synth.s1_params(n)
    res = [n, n, n]
    v, w, g = oracle.new_volume(res)
    for k in (0, 1, 2):
        T = s1_transforms(k, prm)
        oracle.integrate(oracle.scale_depth(synth.s1_frame(k)), v, w, g, res, tranc_dist(prm), 100, T["Rv2c"], T["tv2c"], intr_of(prm),
                         prm["tsdf_voxel_size"])
    T3 = s1_transforms(3, prm)
    v2c = np.eye(4); v2c[:3, :3] = np.asarray(T3["Rv2c"])[..., 0]; v2c[:3, 3] = np.asarray(T3["tv2c"])[..., 0]
    Rs, ts = seeded_poses(np.linalg.inv(v2c))
    ds = torch.from_numpy(oracle.scale_depth(synth.s1_frame(3))).cuda()
    gt = torch.from_numpy(v).cuda()
    ws = torch.zeros(capi.tsdf_reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    out = torch.zeros(32, dtype=torch.float64, device="cuda")
    publish = torch.zeros(capi.gn_publish_bytes() // 8, dtype=torch.float64).pin_memory()
    record = publish.numpy()
    word = record.view(np.uint64)
    mailbox, in_device = capi.icp_mailbox_alloc()
    LEFT = 1 << 63
    common = (ds, W * 4, H, W, intr_of(prm), res, prm["tsdf_voxel_size"])

    def wait(limit_s=30.0):
        t0 = time.perf_counter()
        while int(word[32]) == wait.last and time.perf_counter() - t0 < limit_s:
            pass
        wait.last = int(word[32])
        return wait.last, time.perf_counter() - t0
    wait.last = 0
    ticket = lambda: int(ws[:4].view(torch.int32).item())
    try:
        # poses as arguments, sums published
        capi.tsdf_gauss_newton_terms_ex(*common, Rs, ts, tranc_dist(prm), gt, ws, out, publish_host=publish, publish_seq=11)
        assert wait()[0] == 11
        want = record[:29].copy()
        torch.cuda.synchronize()
        assert want[28] > 1000 and np.array_equal(out.cpu().numpy()[:29], want) and ticket() == 0
        # enqueued ahead: the poses come through the mailbox
        capi.tsdf_gauss_newton_terms_ex(*common, None, None, tranc_dist(prm), gt, ws, out, pose_mailbox=mailbox, mailbox_seq=1, publish_host=publish,
                                        publish_seq=12)
        time.sleep(0.01)
        assert int(word[32]) == 11                                   # (still waiting)
        capi.gn_post_poses(mailbox, Rs, ts, 1)
        assert wait()[0] == 12
        assert np.array_equal(record[:29], want) and record[30] > 0   # ([30]: the ticks it waited)
        torch.cuda.synchronize()
        assert ticket() == 0
        # told to leave
        out.fill_(-1.0)
        capi.tsdf_gauss_newton_terms_ex(*common, None, None, tranc_dist(prm), gt, ws, out, pose_mailbox=mailbox, mailbox_seq=2, publish_host=publish,
                                        publish_seq=13)
        capi.gn_post_poses(mailbox, None, None, 2, cmd=1)
        assert wait()[0] == (13 | LEFT)
        torch.cuda.synchronize()
        assert ticket() == 0 and np.all(out.cpu().numpy() == -1.0)     # nothing summed, nothing written
        # poses that never come: the launch gives up after about a second
        capi.tsdf_gauss_newton_terms_ex(*common, None, None, tranc_dist(prm), gt, ws, out, pose_mailbox=mailbox, mailbox_seq=3, publish_host=publish,
                                        publish_seq=14)
        seen, waited = wait()
        assert seen == (14 | LEFT), (hex(seen), waited)
        torch.cuda.synchronize()
        assert ticket() == 0 and np.all(out.cpu().numpy() == -1.0)
        # ... and the workspace is as good as new
        capi.tsdf_gauss_newton_terms_ex(*common, Rs, ts, tranc_dist(prm), gt, ws, out, publish_host=publish, publish_seq=15)
        assert wait()[0] == 15 and np.array_equal(record[:29], want)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy()[:29], want) and ticket() == 0
        # 512^3: 1024 workgroups, not all resident at once; nobody posts
        big = 512
        gt_big = torch.zeros(big ** 3, dtype=torch.float32, device="cuda")
        capi.tsdf_gauss_newton_terms_ex(ds, W * 4, H, W, intr_of(prm), [big] * 3, prm["tsdf_voxel_size"] * n / big, None, None, tranc_dist(prm), gt_big, ws,
                                        out, pose_mailbox=mailbox, mailbox_seq=4, publish_host=publish, publish_seq=16)
        seen, waited = wait()
        torch.cuda.synchronize()
        assert seen == (16 | LEFT) and ticket() == 0
        first = waited
        capi.tsdf_gauss_newton_terms_ex(*common, None, None, tranc_dist(prm), gt, ws, out, pose_mailbox=mailbox, mailbox_seq=5, publish_host=publish,
                                        publish_seq=17)
        seen, one_wave = wait()
        assert seen == (17 | LEFT)
        torch.cuda.synchronize()
        assert first < 1.6 * one_wave + 0.2, (first, one_wave)       # (one time-out, not one per round of resident workgroups)
    finally:
        torch.cuda.synchronize()
        capi.icp_mailbox_free(mailbox, in_device)


def test_relocalize_recovers_a_perturbed_pose(dev):
    """Map from six frames, then the last frame's pose is perturbed (4 cm at the camera, 0.5 degrees) and refined
    against the map: the mean squared residual falls monotonically to less than half and the camera moves back
    towards the tracked pose.  (Plane + sphere leaves sliding along the plane weakly constrained, and the tracked
    pose is ICP's optimum, not this residual's: exact recovery is not the claim.)"""
    torch, _, pl = dev
    n = 128
    prm = synth.s1_params(n)
    kf = pl.KinectFusion(prm)
    frames = [torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda() for k in range(6)]
    for k in range(6):
        assert kf.process_frame(frames[k]) == 1
    truth = kf.camera2volume()
    t_true = truth[..., 0].astype(np.float64)
    xi = np.array([0.008, -0.006, 0.005, 0.004, -0.005, 0.006])
    start = twist_matrix(xi) @ t_true
    c2v0 = np.zeros((4, 4, 2), np.float32); c2v0[..., 0] = start
    terms = kf.gauss_newton_terms(frames[5], c2v0)
    assert terms is not None and terms[28] > 1000
    ok, refined, hist = kf.relocalize(frames[5], c2v0, iterations=6, damping=1e-3)
    assert ok
    assert np.all(np.diff(hist) <= 1e-9) and hist[-1] < 0.5 * hist[0]
    def err(m):
        d = np.linalg.inv(t_true) @ m
        return np.linalg.norm(d[:3, 3]), np.arccos(np.clip((np.trace(d[:3, :3]) - 1) / 2, -1, 1))
    e0, e1 = err(start), err(refined[..., 0].astype(np.float64))
    assert e1[0] < 0.7 * e0[0] and e1[1] < 1.3 * e0[1], (e0, e1)
    assert np.all(refined[..., 1] == 0)
    kf.close()


def se3_exp_c64(xi):
    """The reference's se3Exp (KinectFusionReconstruction.h:176-219) restated in numpy complex64, operation for operation: the hat matrix,
    the small-angle branch on |omega| < 1e-6, A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3 with t = sqrt(omega^T omega)
    (no conjugation), R = I + A K + B K^2, V = I + B K + C K^2, translation V v."""
    xi = np.asarray(xi, np.complex64)
    v, om = xi[:3], xi[3:]
    K = np.zeros((3, 3), np.complex64)
    K[0, 1], K[0, 2], K[1, 2] = -om[2], om[1], -om[0]
    K[1, 0], K[2, 0], K[2, 1] = om[2], -om[1], om[0]
    I = np.eye(3, dtype=np.complex64)
    if np.sqrt(np.sum(np.abs(om) ** 2)) < 1e-6:
        R, V = I + K, I + K
    else:
        th = np.sqrt(np.complex64(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]))
        s_, c_ = np.sin(th), np.cos(th)
        K2 = (K @ K).astype(np.complex64)
        A = np.complex64(s_ / th); B = np.complex64((np.complex64(1) - c_) / th ** 2); Cc = np.complex64((th - s_) / th ** 3)
        R, V = I + A * K + B * K2, I + B * K + Cc * K2
    T = np.zeros((4, 4), np.complex64)
    T[:3, :3] = R; T[:3, 3] = V @ v; T[3, 3] = 1
    return T


def test_relocalization_loop_against_an_oracle_twin(dev, oracle):
    """RelocalizeGaussNewton as a loop (the per-pass kernel had an oracle twin, the host's damped solve + se3Exp step
    did not).  The twin: the oracle's six-pose kernel for the 29 sums, and around it a numpy restatement of the host step — poses
    inverse(se3Exp(i h e_k) c2v) in complex64, sums scaled by 1 / h and 1 / h^2, the damped 6x6 system solved by Cholesky in double,
    the update se3Exp(x) c2v in complex64 (se3Exp restated from the reference's text, above).  Five iterations at 128^3 (scene S3) from a
    perturbed pose: every intermediate loss and the final camera2volume agree (pose entries within 1e-6)."""
    torch, capi, pl = dev
    n = 128
    prm = synth.s1_params(n)
    kf = pl.KinectFusion(prm)
    frames = [synth.s3_frame(k) for k in range(6)]   # the box room: every degree of freedom constrained, so rounding differences are not amplified
    dfr = [torch.from_numpy(f.view(np.int16)).cuda() for f in frames]
    for k in range(6):
        assert kf.process_frame(dfr[k]) == 1
    t_true = kf.camera2volume()[..., 0].astype(np.float64)
    start = twist_matrix(np.array([0.008, -0.006, 0.005, 0.004, -0.005, 0.006])) @ t_true
    c2v0 = np.zeros((4, 4, 2), np.float32); c2v0[..., 0] = start
    iters, damping = 5, 1e-3
    ok, refined, hist = kf.relocalize(dfr[5], c2v0, iterations=iters, damping=damping)
    assert ok
    gt = kf.volume()[0]                     # the map the GPU loop aligned to (value plane, dense)
    kf.close()
    ds = oracle.scale_depth(frames[5])
    res, vs, trunc, k4 = [n, n, n], prm["tsdf_voxel_size"], tranc_dist(prm), intr_of(prm)
    h = np.float32(1e-7)
    c2v = (c2v0[..., 0] + 1j * c2v0[..., 1]).astype(np.complex64)
    twin_hist = []
    def terms(c2v):
        Rs = np.zeros((6, 3, 3, 2), np.float32); ts = np.zeros((6, 3, 2), np.float32)
        for k in range(6):
            xi = np.zeros(6, np.complex64); xi[k] = 1j * h
            v2c = np.linalg.inv((se3_exp_c64(xi) @ c2v).astype(np.complex128)).astype(np.complex64)
            Rs[k, ..., 0], Rs[k, ..., 1] = v2c[:3, :3].real, v2c[:3, :3].imag
            ts[k, :, 0], ts[k, :, 1] = v2c[:3, 3].real, v2c[:3, 3].imag
        s = oracle.tsdf_gn_terms(ds, res, vs, Rs, ts, trunc, k4, gt)
        ih = 1.0 / float(h)
        s = s.copy(); s[:21] *= ih * ih; s[21:27] *= ih
        return s
    for it in range(iters):
        s = terms(c2v)
        twin_hist.append(s[27] / s[28])
        A = np.zeros((6, 6)); q = 0
        for j in range(6):
            for k in range(j, 6):
                A[j, k] = A[k, j] = s[q]; q += 1
        A[np.diag_indices(6)] *= 1.0 + float(np.float32(damping))
        L = np.linalg.cholesky(A)
        x = np.linalg.solve(L.T, np.linalg.solve(L, -s[21:27]))
        c2v = (se3_exp_c64(x.astype(np.float32).astype(np.complex64)) @ c2v).astype(np.complex64)
    s = terms(c2v)
    twin_hist.append(s[27] / s[28])
    assert np.all(np.abs(refined[..., 0] - c2v.real) <= 1e-6), np.abs(refined[..., 0] - c2v.real).max()
    assert np.all(refined[..., 1] == 0) and np.all(c2v.imag == 0)
    assert np.allclose(hist, twin_hist, rtol=2e-4, atol=0), (hist, twin_hist)
    assert hist[-1] < 0.5 * hist[0]


def test_relocalize_loop_protocol_changes_no_bit(dev):
    """Round 6: the loop's passes are enqueued ahead of their poses (mailbox), their sums published to pinned memory by the kernel's last
    workgroup, the depth scaled once per frame.  The same refinement with gn_post_pose false (every pass launched with its poses as arguments,
    after the solve): identical camera2volume and loss history, bit for bit, over five frames; and a loop that ends early — an empty map: nothing
    to align to on its first pass, while the second pass's kernel is already waiting for poses — tells that kernel to leave, returns failure, and
    the next call on the same object is unaffected (no stale poses, no stale record)."""
    torch, capi, pl = dev
    n = 128
    runs = {}
    for posted in (True, False):
        kf = pl.KinectFusion(dict(synth.s1_params(n), gn_post_pose=posted))
        dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(9)]
        empty_fail = kf.relocalize(dfr[0], kf.camera2volume(), iterations=5)[0]      # (before any frame: the map is empty)
        for k in range(4):
            assert kf.process_frame(dfr[k]) == 1
        t_true = kf.camera2volume()[..., 0].astype(np.float64)
        out = []
        for k in range(4, 9):
            start = twist_matrix(np.array([0.006, -0.004, 0.005, 0.003, -0.004, 0.005]) * (1 + 0.1 * k)) @ t_true
            c2v0 = np.zeros((4, 4, 2), np.float32); c2v0[..., 0] = start
            ok, refined, hist = kf.relocalize(dfr[k], c2v0, iterations=5, damping=1e-3)
            assert ok and hist[-1] < hist[0]
            ok1, refined1, hist1 = kf.relocalize(dfr[k], c2v0, iterations=1, damping=1e-3)    # (a loop of two passes, then one without history: one pass)
            assert ok1 and np.array_equal(hist1, hist[:2])
            out.append((refined, hist))
        times = kf.gn_times()
        assert times["passes"] == 1 + 5 * (6 + 2)    # (the pass on the empty map was seen too)
        kf.close()
        runs[posted] = (empty_fail, out)
    assert runs[True][0] is False and runs[False][0] is False
    for (ra, ha), (rb, hb) in zip(runs[True][1], runs[False][1]):
        assert np.array_equal(ra.view(np.int32), rb.view(np.int32)) and np.array_equal(ha, hb)


def test_residual_kernels_non_cubic_volume(dev, oracle):
    """The three residual kernels (dual-complex Hessian, real loss, six-pose Gauss-Newton terms) over a 96 x 64 x 80 map —
    two columns of 64-wide tiles, the second a half one; planes that are not a multiple of the 32-plane batches — against
    the oracle, whole and as two unequal slabs."""
    torch, capi, _ = dev
    prm = synth.s1_params(96)
    res = [96, 64, 80]
    X, Y, Z = res
    v, w, g = oracle.new_volume(res)
    for k in (0, 1, 2):
        T = s1_transforms(k, prm)
        oracle.integrate(oracle.scale_depth(synth.s1_frame(k)), v, w, g, res, tranc_dist(prm), 100, T["Rv2c"], T["tv2c"], intr_of(prm),
                         prm["tsdf_voxel_size"])
    T3 = s1_transforms(3, prm)
    ds = oracle.scale_depth(synth.s1_frame(3))
    dds, gt = torch.from_numpy(ds).cuda(), torch.from_numpy(v).cuda()
    ws = torch.zeros(capi.tsdf_reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    trunc, vs, k4 = tranc_dist(prm), prm["tsdf_voxel_size"], intr_of(prm)
    # dual-complex pose: value, seed 1e-6 on t_x in both first-order slots
    Rd = np.zeros((3, 3, 4), np.float32); td = np.zeros((3, 4), np.float32)
    Rd[..., 0] = np.asarray(T3["Rv2c"])[..., 0]; td[..., 0] = np.asarray(T3["tv2c"])[..., 0]; td[0, 1] = 1e-6; td[0, 2] = 1e-6
    want4 = oracle.tsdf_hessian(ds, res, vs, Rd, td, trunc, k4, v)
    want4 = want4[0] if isinstance(want4, tuple) else want4
    out4 = torch.zeros(4, dtype=torch.float64, device="cuda")
    def hess(z0, z1):
        out4.zero_()
        capi.compute_local_tsdf_hessian(dds, W * 4, H, W, k4, res, vs, Rd, td, trunc, gt[z0 * X * Y:], ws, out4, z0=z0, z1=z1)
        torch.cuda.synchronize()
        return out4.cpu().numpy().copy()
    got4 = hess(0, Z)
    assert want4[3] > 1000 and got4[3] == want4[3]
    assert abs(got4[0] - want4[0]) <= 1e-6 * abs(want4[0]) and abs(got4[1] - want4[1]) <= 1e-6 * abs(want4[1])
    assert abs(got4[2] - want4[2]) <= 1e-5 * abs(want4[2])
    parts = hess(0, 37) + hess(37, Z)
    assert parts[3] == got4[3] and np.allclose(parts, got4, rtol=1e-11)
    # real loss
    R9, t3 = Rd[..., 0].reshape(9), td[..., 0].reshape(3)
    wl = oracle.tsdf_loss(ds, res, vs, R9, t3, trunc, k4, v)
    out2 = torch.zeros(2, dtype=torch.float64, device="cuda")
    capi.compute_local_tsdf_loss(dds, W * 4, H, W, k4, res, vs, R9, t3, trunc, gt, ws, out2)
    torch.cuda.synchronize()
    gl = out2.cpu().numpy()
    assert gl[1] == wl[1] and abs(gl[0] - wl[0]) <= 1e-6 * abs(wl[0])
    # Gauss-Newton terms
    v2c = np.eye(4); v2c[:3, :3] = Rd[..., 0]; v2c[:3, 3] = td[..., 0]
    Rs, ts = seeded_poses(np.linalg.inv(v2c))
    want = oracle.tsdf_gn_terms(ds, res, vs, Rs, ts, trunc, k4, v)
    out = torch.zeros(32, dtype=torch.float64, device="cuda")
    capi.tsdf_gauss_newton_terms(dds, W * 4, H, W, k4, res, vs, Rs, ts, trunc, gt, ws, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()[:29]
    assert got[28] == want[28] > 1000 and np.allclose(got[27], want[27], rtol=1e-9)
    assert np.all(np.abs(got[:21] - want[:21]) <= 1e-6 * np.abs(want[:21]).max())
    assert np.all(np.abs(got[21:27] - want[21:27]) <= 1e-6 * np.abs(want[21:27]).max())


def test_residual_kernels_random_shapes_poses_and_slabs(dev, oracle):
    """Round 6 rewrote the residual kernels' scan (sixteen bytes per lane, interleaved z groups, nontemporal loads; the one-column form where a
    row is no multiple of 16 bytes or the map is not 16-byte aligned).  Ten seeded trials: a volume of random extent (rows of 90 .. 100 voxels,
    most of them no multiple of four), a randomly perturbed pose, a random dual seed — Hessian, loss and Gauss-Newton sums against the ORACLE over
    the whole map, over three random slabs (whose plane counts pick one, two, three or five z groups), and over the same map at an address that
    is only 4-byte aligned (the one-column scan): counts exact, sums to the tolerances of the fixed-shape tests; the two scan forms agree with each
    other to double rounding."""
    torch, capi, _ = dev
    rng = np.random.default_rng(20261004)
    prm = synth.s1_params(96)
    trunc, vs, k4 = tranc_dist(prm), prm["tsdf_voxel_size"], intr_of(prm)
    ws = torch.zeros(capi.tsdf_reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    out4 = torch.zeros(4, dtype=torch.float64, device="cuda")
    out2 = torch.zeros(2, dtype=torch.float64, device="cuda")
    out = torch.zeros(32, dtype=torch.float64, device="cuda")
    widths_seen = set()
    for trial in range(10):
        X, Y, Z = int(rng.integers(90, 101)), int(rng.integers(60, 73)), int(rng.integers(70, 97))
        if trial == 0:
            X = 96      # (at least one wide case and one narrow one whatever the generator gives)
        if trial == 1:
            X = 97
        widths_seen.add(X % 4 == 0)
        res = [X, Y, Z]
        v, w, g = oracle.new_volume(res)
        for k in (0, 1):
            T = s1_transforms(k, prm)
            oracle.integrate(oracle.scale_depth(synth.s1_frame(k)), v, w, g, res, trunc, 100, T["Rv2c"], T["tv2c"], k4, vs)
        T2 = s1_transforms(2, prm)
        v2c = np.eye(4); v2c[:3, :3] = np.asarray(T2["Rv2c"])[..., 0]; v2c[:3, 3] = np.asarray(T2["tv2c"])[..., 0]
        v2c = np.linalg.inv(twist_matrix(rng.normal(size=6) * [0.01, 0.01, 0.01, 0.004, 0.004, 0.004]) @ np.linalg.inv(v2c))
        ds = oracle.scale_depth(synth.s1_frame(2))
        dds = torch.from_numpy(ds).cuda()
        store = torch.zeros(X * Y * Z + 5, dtype=torch.float32, device="cuda")   # the map at a 16-byte aligned address and at one that is not
        aligned, shifted = store[4:4 + X * Y * Z], store[5:5 + X * Y * Z]
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
        Rd = np.zeros((3, 3, 4), np.float32); td = np.zeros((3, 4), np.float32)
        Rd[..., 0] = v2c[:3, :3]; td[..., 0] = v2c[:3, 3]
        dof = int(rng.integers(0, 3)); td[dof, 1] = 1e-6; td[dof, 2] = 1e-6
        R9, t3 = Rd[..., 0].reshape(9).copy(), td[..., 0].reshape(3).copy()
        Rs, ts = seeded_poses(np.linalg.inv(v2c.astype(np.float32).astype(np.float64)))
        cuts = sorted(int(c) for c in rng.choice(np.arange(8, Z - 8), size=2, replace=False))
        slabs = [(0, Z), (0, cuts[0]), (cuts[0], cuts[1]), (cuts[1], Z)]

        def run(gt, z0, z1):
            out4.zero_(); out2.zero_(); out.zero_()
            capi.compute_local_tsdf_hessian(dds, W * 4, H, W, k4, res, vs, Rd, td, trunc, gt[z0 * X * Y:], ws, out4, z0=z0, z1=z1)
            capi.compute_local_tsdf_loss(dds, W * 4, H, W, k4, res, vs, R9, t3, trunc, gt[z0 * X * Y:], ws, out2, z0=z0, z1=z1)
            capi.tsdf_gauss_newton_terms(dds, W * 4, H, W, k4, res, vs, Rs, ts, trunc, gt[z0 * X * Y:], ws, out, z0=z0, z1=z1)
            torch.cuda.synchronize()
            return out4.cpu().numpy().copy(), out2.cpu().numpy().copy(), out.cpu().numpy()[:29].copy()

        for z0, z1 in slabs:
            sl = v[z0 * X * Y:z1 * X * Y]
            w4 = oracle.tsdf_hessian(ds, res, vs, Rd, td, trunc, k4, sl, z0=z0, z1=z1)
            w4 = w4[0] if isinstance(w4, tuple) else w4
            w2 = oracle.tsdf_loss(ds, res, vs, R9, t3, trunc, k4, v, z0=z0, z1=z1)     # (this wrapper takes the whole map and absolute planes)
            w29 = oracle.tsdf_gn_terms(ds, res, vs, Rs, ts, trunc, k4, sl, z0=z0, z1=z1)
            results = []
            for gt in (aligned, shifted):
                gt.copy_(torch.from_numpy(v))
                g4, g2, g29 = run(gt, z0, z1)
                results.append((g4, g2, g29))
                tag = (trial, res, (z0, z1), gt.data_ptr() % 16)
                assert g4[3] == w4[3] and g2[1] == w2[1] and g29[28] == w29[28], tag
                if w4[3] > 0:
                    assert abs(g4[0] - w4[0]) <= 1e-6 * abs(w4[0]) and abs(g4[1] - w4[1]) <= 1e-6 * max(abs(w4[1]), 1e-3 * abs(w4[0])), tag
                    assert abs(g4[2] - w4[2]) <= 1e-5 * max(abs(w4[2]), 1e-3 * abs(w4[0])), tag
                    assert abs(g2[0] - w2[0]) <= 1e-6 * abs(w2[0]), tag
                if w29[28] > 0:
                    assert np.allclose(g29[27], w29[27], rtol=1e-9), tag
                    assert np.all(np.abs(g29[:21] - w29[:21]) <= 1e-6 * np.abs(w29[:21]).max()), tag
                    assert np.all(np.abs(g29[21:27] - w29[21:27]) <= 1e-6 * np.abs(w29[21:27]).max()), tag
            for a, b in zip(*results):   # sixteen bytes per lane against one column per lane: the same voxels, another order of the double sums
                assert np.allclose(a, b, rtol=1e-10, atol=1e-13 * max(np.abs(a).max(), 1e-30))
            if (z0, z1) == (0, Z):
                assert w4[3] > 200 and w29[28] > 200, (trial, res, w4[3], w29[28])
    assert widths_seen == {True, False}


def test_gn_terms_full_size_1024_eight_slabs(dev):
    """BASELINE config 5's size: a 1024^3 volume (two S1 frames fused into it on the GPU), then the
    Gauss-Newton terms of the next frame over the whole volume and over the eight z-slabs an 8-GPU run
    gives its ranks.  Size-independent properties: the slab counts add up exactly, the 28 sums add up to
    double rounding (what the ranks all-reduce), a second launch returns the same bits, J^T J is positive
    semi-definite, and the band holds a sensible share of the volume."""
    torch, capi, _ = dev
    n = 1024
    prm = synth.s1_params(n)
    res = [n, n, n]
    value = torch.zeros((n * n, n), dtype=torch.float32, device="cuda")
    weight = torch.zeros((n * n, n), dtype=torch.int32, device="cuda")
    grad = torch.zeros((n * n, n), dtype=torch.float32, device="cuda")
    scaled = torch.empty((H, W), dtype=torch.float32, device="cuda")
    dmax = torch.zeros(1, dtype=torch.float32, device="cuda")
    iws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    upd = torch.zeros(1, dtype=torch.int64, device="cuda")
    for k in (0, 1):
        T = s1_transforms(k, prm)
        depth = torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda()
        dmax.zero_()
        capi.scale_depth_max(depth, W * 2, H, W, scaled, W * 4, dmax)
        capi.integrate_scaled(scaled, W * 4, H, W, intr_of(prm), 100, res, prm["tsdf_voxel_size"], T["Rv2c"], T["tv2c"], tranc_dist(prm),
                              value, weight, grad, n * 4, z0=0, z1=n, updated=upd, depth_max=dmax, workspace=iws)
    torch.cuda.synchronize()
    assert int(upd.item()) > 10_000_000       # 8x the voxels of the 512^3 run's ~1.9 M per frame, two frames
    del weight, grad
    T2 = s1_transforms(2, prm)
    v2c = np.eye(4); v2c[:3, :3] = np.asarray(T2["Rv2c"])[..., 0]; v2c[:3, 3] = np.asarray(T2["tv2c"])[..., 0]
    Rs, ts = seeded_poses(np.linalg.inv(v2c))
    depth = torch.from_numpy(synth.s1_frame(2).view(np.int16)).cuda()
    capi.scale_depth_max(depth, W * 2, H, W, scaled, W * 4, dmax)
    ws = torch.zeros(capi.tsdf_reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    out = torch.zeros(32, dtype=torch.float64, device="cuda")

    def terms(z0, z1):
        out.zero_()
        capi.tsdf_gauss_newton_terms(scaled, W * 4, H, W, intr_of(prm), res, prm["tsdf_voxel_size"], Rs, ts, tranc_dist(prm),
                                     value[z0 * n:], ws, out, z0=z0, z1=z1)
        torch.cuda.synchronize()
        return out.cpu().numpy()[:29].copy()

    whole = terms(0, n)
    assert np.array_equal(whole, terms(0, n))
    parts = np.zeros(29)
    for r in range(8):
        parts += terms(r * n // 8, (r + 1) * n // 8)
    assert parts[28] == whole[28] and whole[28] > 500_000
    assert np.allclose(parts[:28], whole[:28], rtol=1e-9, atol=1e-11 * np.abs(whole[:28]).max())
    JtJ = np.zeros((6, 6))
    JtJ[np.triu_indices(6)] = whole[:21]
    JtJ = JtJ + np.triu(JtJ, 1).T
    assert np.linalg.eigvalsh(JtJ).min() >= -1e-9 * np.abs(JtJ).max()
    assert whole[27] >= 0
