"""Scoring many pose hypotheses in one pass over the band index and global relocalisation, measured on
  - bench.py's reloc scene: S3 with 7-Scenes intrinsics at 1024^3, a map of four frames;
  - scene S1 at 512^3, a map of four tracked frames.
Reports per scene
  - the index build and its size;
  - kernel time (hipEvent pairs) of ONE launch of xs_tsdf_score_poses_band at P = 64, 512, 4096 — Halton hypotheses in a 0.9 m / 0.9 rad box
    round a start 0.88 m and 51 degrees off the next frame's pose — against P launches of the dense xs_compute_local_tsdf_loss at the same
    poses, same map, same process (the only way before this kernel), and the largest difference of the two results;
  - the wall clock of a whole KinectFusion.relocalize_global at P = 2048, keep 8, 10 iterations, and where it ends.
No ratio is a condition; the exit status is 1 only if a count differs or a sum leaves the bound 8 * 2^-24.  Run in its own process:
    python profiles/tools/probe_score_poses.py > profiles/score_poses_probe.txt"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_newton import timed  # noqa: E402  (profiles/tools: hipEvent pairs, median after a warm-up)


def scene(name, n):
    import torch
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    nmap = 4
    if name == "reloc":     # bench.py reloc_workload's setup
        gtp = np.zeros((nmap, 4, 4, 2), np.float32)
        for k in range(nmap):
            gtp[k, ..., 0] = synth.s1_pose(k)
        prm = dict(synth.s1_params(n, seed=None), flag_use_gtPose=True, **synth.SEVEN_SCENES)
        frame = lambda k: synth.s3_frame(k, **synth.SEVEN_SCENES)
        kf = pl.KinectFusion(prm, gt_poses=gtp)
    else:
        prm = synth.s1_params(n, seed=None)
        frame = synth.s1_frame
        kf = pl.KinectFusion(prm)
    for k in range(nmap):
        assert kf.process_frame(torch.from_numpy(frame(k).view(np.int16)).cuda()) == 1
    kf.synchronize()
    query = torch.from_numpy(frame(nmap).view(np.int16)).cuda()
    w2v = np.eye(4); w2v[:3, 3] = [prm["init_x"], prm["init_y"], prm["init_z"]]
    return kf, prm, query, w2v @ synth.s1_pose(nmap)


def main(name, n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    sh = importlib.import_module("x-slam_amd.sharded")
    from helpers import intr_of, tranc_dist
    import score_cases as sc

    kf, prm, query, truth = scene(name, n)
    W, H = synth.WIDTH, synth.HEIGHT
    print(f"---- scene {name}, {n}^3, map of 4 frames, one MI355X")
    p, step = kf.volume_ptr("value")
    assert step == n * 4, "the probe reads the value array as the dense map"
    gt = torch.as_tensor(sh._DevView(p, n * n * n, "<f4"), device="cuda")
    res = [n, n, n]
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = capi.tsdf_band_build(gt, res)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    nchunks = (idx.count + 63) // 64
    print(f"index: {idx.count} band voxels ({idx.count * 12 / 2**20:.1f} MiB of keys + values), {nchunks} chunks of 64 on "
          f"{min(1024, max(1, (nchunks + 3) // 4))} workgroups per tile of 64 poses; build through capi (count call + fill call): {min(times):.1f} ms (best of 3)")

    k4, vs, trunc = intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm)
    scaled = torch.empty((H, W), dtype=torch.float32, device="cuda")
    capi.scale_depth(query, W * 2, H, W, scaled, W * 4)
    start = sc.global_start(truth)
    t0 = time.perf_counter()
    cands = pl.pose_candidates(start, sc.GLOBAL_BOX_T, sc.GLOBAL_BOX_R, 4096)
    print(f"pose_candidates(start, 0.9, 0.9, 4096) on the host: {(time.perf_counter() - t0) * 1e3:.0f} ms")
    Rt = [sc.v2c_f32(m) for m in cands[..., 0].astype(np.float64)]
    R, t = np.stack([r for r, _ in Rt]), np.stack([x for _, x in Rt])
    ws = torch.zeros(capi.tsdf_reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    sws = torch.zeros(capi.tsdf_score_poses_workspace_bytes(capi.SCORE_MAX_POSES), dtype=torch.uint8, device="cuda")
    out = torch.zeros(2 * capi.SCORE_MAX_POSES, dtype=torch.float64, device="cuda")
    dense = torch.zeros((capi.SCORE_MAX_POSES, 2), dtype=torch.float64, device="cuda")
    good = True
    print("kernel time (hipEvent pairs around the launches; the one-launch figures include the pose upload, 48 B per pose):")
    for P in (64, 512, 4096):
        def dense_launches():
            for q in range(P):
                capi.compute_local_tsdf_loss(scaled, W * 4, H, W, k4, res, vs, R[q], t[q], trunc, gt, ws, dense[q])
        reps = 5 if P == 64 else 1
        d = timed(torch, dense_launches, reps=reps)
        one = timed(torch, lambda: capi.tsdf_score_poses_band(scaled, W * 4, H, W, k4, vs, R[:P], t[:P], trunc, idx, sws, out), reps=20)
        torch.cuda.synchronize()
        a, b = out[:2 * P].cpu().numpy().reshape(P, 2), dense[:P].cpu().numpy()
        same = bool(np.array_equal(a[:, 1], b[:, 1]))
        rel = float((np.abs(a[:, 0] - b[:, 0]) / np.where(b[:, 0] > 0, b[:, 0], 1.0)).max())
        good = good and same and rel <= sc.SUM_BOUND
        print(f"  P = {P:4d}: one launch {one * 1e3:8.0f} us ({one * 1e3 / P:6.2f} us per pose, median of 20); {P} dense launches {d * 1e3:9.0f} us "
              f"({d * 1e3 / P:.0f} us each, {'median of 5' if reps > 1 else 'one run after a warm-up'}): {d / one:.0f} x; counts equal: {same}, "
              f"largest |sum - dense| / dense {rel:.2e} (bound {sc.SUM_BOUND:.2e}); poses in view {int((b[:, 1] > 0).sum())}, largest count {b[:, 1].max():.0f}")
    del idx, gt

    # ---- the whole search
    cand = cands[:sc.GLOBAL_CANDIDATES]
    s_t, c_t = kf.score_poses(query, sc.as_c2v32(np.stack([truth, start])))
    kf.relocalize_global(query, cand, keep=sc.GLOBAL_KEEP, iterations=sc.GLOBAL_ITERATIONS, damping=sc.GLOBAL_DAMPING)
    wall = []
    for _ in range(5):
        t0 = time.perf_counter()
        ok, best, rep = kf.relocalize_global(query, cand, keep=sc.GLOBAL_KEEP, iterations=sc.GLOBAL_ITERATIONS, damping=sc.GLOBAL_DAMPING)
        wall.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    kf.score_poses(query, cand)
    score_ms = (time.perf_counter() - t0) * 1e3
    ok0, end0, _ = kf.relocalize(query, sc.as_c2v32(start), iterations=sc.GLOBAL_ITERATIONS)
    err = sc.pose_error(best[..., 0], truth)
    print(f"relocalize_global, {sc.GLOBAL_CANDIDATES} candidates round a start {sc.pose_error(start, truth)[0]:.3f} m / {sc.pose_error(start, truth)[1]:.1f} deg off, "
          f"keep {sc.GLOBAL_KEEP}, {sc.GLOBAL_ITERATIONS} iterations: {np.median(wall):.2f} ms wall clock (median of 5; score_poses of the {sc.GLOBAL_CANDIDATES} alone, "
          f"host side included: {score_ms:.2f} ms)")
    print(f"  ok {ok}, winner {err[0] * 1e3:.2f} mm / {err[1]:.3f} deg from the synthetic pose; S at that pose {sc.S(s_t[0], c_t[0]):.1f}, at the start "
          f"{sc.S(s_t[1], c_t[1]):.1f}; report {rep}")
    print(f"  relocalize (Gauss-Newton) from the start itself: ok {ok0}, ends {sc.pose_error(end0[..., 0], truth)[0]:.3f} m off")
    kf.close()
    return good


if __name__ == "__main__":
    which = sys.argv[1:] or ["reloc:1024", "s1:512"]
    good = True
    for w in which:
        name, n = w.split(":")
        good = main(name, int(n)) and good
    if not good:
        print("DEFECT: a count differs from the dense launch's or a sum leaves the bound")
    sys.exit(0 if good else 1)
