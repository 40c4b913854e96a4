"""The exact pose Hessian in one pass over the band index and Newton relocalisation, measured on
  - bench.py's reloc scene: S3 with 7-Scenes intrinsics at 1024^3, a map of four frames, bench.py's perturbed starts (0.3 deg, ~1 cm);
  - scene S1 at 512^3, a map of four tracked frames, the same offset.
Reports per scene
  - the index build and its size;
  - kernel time (hipEvent pairs, median of 20 after a warm-up) of ONE launch of xs_tsdf_pose_hessian_band at F = 1, 4, 16 and of the 21
    launches of the dense single-pair kernel xs_compute_local_tsdf_hessian that give the same 6 x 6 matrix, same map, same process;
  - the loops: passes and wall clock of relocalize(method="newton") and of relocalize (Gauss-Newton) from the same starts to the same
    final loss, and the fallback count.
The only condition: the single launch at F = 1 is faster than the 21 launches (exit status 1 otherwise).  Run in its own process:
    python profiles/tools/probe_newton.py > profiles/newton_probe.txt"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scene(name, n):
    import torch
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    nmap, F = 4, 16
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
    frames = [torch.from_numpy(frame(nmap + k).view(np.int16)).cuda() for k in range(F)]
    w2v = np.eye(4); w2v[:3, 3] = [prm["init_x"], prm["init_y"], prm["init_z"]]
    off = np.eye(4)
    a = np.radians(0.3)
    off[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    off[:3, 3] = [0.006, -0.005, 0.006]
    starts = [synth.cmat(w2v @ synth.s1_pose(nmap + k) @ off) for k in range(F)]
    return kf, prm, frames, starts


def timed(torch, fn, reps=20):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def passes_to(hist, target):
    """Steps after which the loss history is at or below target (len(hist) - 1 if never)."""
    hit = np.nonzero(np.asarray(hist) <= target)[0]
    return int(hit[0]) if hit.size else len(hist) - 1


def main(name, n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    synth = importlib.import_module("x-slam_amd.synth")
    sh = importlib.import_module("x-slam_amd.sharded")
    from helpers import intr_of, tranc_dist
    import newton_cases as nc

    kf, prm, frames, starts = scene(name, n)
    F = len(frames)
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
          f"{min(4096, max(1, (nchunks + 3) // 4))} workgroups per frame; build through capi (count call + fill call): {min(times):.1f} ms (best of 3)")

    k4, vs, trunc = intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm)
    scaled = [torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(F)]
    for f in range(F):
        capi.scale_depth(frames[f], W * 2, H, W, scaled[f], W * 4)
    poses = [nc.pair_poses(nc.v2c_of(s[..., 0])) for s in starts]
    ws = torch.zeros(capi.tsdf_reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    nws = torch.zeros(capi.tsdf_pose_hessian_workspace_bytes(capi.BAND_MAX_FRAMES), dtype=torch.uint8, device="cuda")
    out = torch.zeros(29 * capi.BAND_MAX_FRAMES, dtype=torch.float64, device="cuda")
    out4 = torch.zeros(4, dtype=torch.float64, device="cuda")

    def dense21():
        for q in range(21):
            capi.compute_local_tsdf_hessian(scaled[0], W * 4, H, W, k4, res, vs, poses[0][0][q], poses[0][1][q], trunc, gt, ws, out4)

    d21 = timed(torch, dense21)
    print("kernel time, median of 20 (hipEvent pairs around the launches; the one-launch figures include the 4 KB pose upload per frame):")
    print(f"  21 launches of the dense single-pair kernel (xs_compute_local_tsdf_hessian): {d21 * 1e3:.0f} us ({d21 * 1e3 / 21:.0f} us each)")
    one = {}
    for nf in (1, 4, 16):
        R, t = np.stack([poses[f][0] for f in range(nf)]), np.stack([poses[f][1] for f in range(nf)])
        one[nf] = timed(torch, lambda: capi.tsdf_pose_hessian_band(scaled[:nf], W * 4, H, W, k4, vs, R, t, trunc, idx, nws, out))
        print(f"  one launch over the index, F = {nf:2d}: {one[nf] * 1e3:.0f} us per launch, {one[nf] * 1e3 / nf:.0f} us per frame")
    print(f"  one launch (F = 1) against the 21 launches: {d21 / one[1]:.2f} x faster; with the index build: {(one[1] + min(times)) * 1e3:.0f} us the first time")
    torch.cuda.synchronize()
    cnt = float(out[28].item())
    del idx, gt

    # ---- the loops, same starts: losses per pass, passes and wall clock to the same final loss
    iters = 8
    ok_n, _, hist_n, fb = kf.relocalize_batch(frames, np.stack(starts), iterations=iters, method="newton")
    ok_g, _, hist_g = kf.relocalize_batch(frames, np.stack(starts), iterations=iters)
    assert ok_n.all() and ok_g.all()
    target = np.maximum(hist_n[:, -1], hist_g[:, -1]) * 1.001
    pn = [passes_to(hist_n[f], target[f]) for f in range(F)]
    pg = [passes_to(hist_g[f], target[f]) for f in range(F)]
    print(f"loops from the same {F} starts, {iters} iterations, count {cnt:.0f}: fallbacks {int(fb.sum())}")
    print(f"  frame 0 losses, Newton:       {np.array2string(hist_n[0], precision=4)}")
    print(f"  frame 0 losses, Gauss-Newton: {np.array2string(hist_g[0], precision=4)}")
    print(f"  steps to the common final loss (the larger of the two final losses + 0.1 %): Newton {np.mean(pn):.2f} (max {max(pn)}), "
          f"Gauss-Newton {np.mean(pg):.2f} (max {max(pg)}), mean over the frames")

    def wall(method, steps):
        def run():
            for f in range(F):
                r = kf.relocalize(frames[f], starts[f], iterations=steps[f], method=method)
                assert r[0]
        run()
        best = []
        for _ in range(5):
            t0 = time.perf_counter(); run(); best.append(time.perf_counter() - t0)
        return float(np.median(best)) / F * 1e3

    wn, wg = wall("newton", pn), wall("gauss_newton", pg)
    print(f"  wall clock per relocalisation to that loss (steps as above + the final loss pass, median of 5 runs of {F} frames): "
          f"Newton {wn:.2f} ms, Gauss-Newton {wg:.2f} ms")
    bn = []
    for method in ("newton", "gauss_newton"):
        kf.relocalize_batch(frames, np.stack(starts), iterations=5, method=method)
        best = []
        for _ in range(5):
            t0 = time.perf_counter(); kf.relocalize_batch(frames, np.stack(starts), iterations=5, method=method); best.append(time.perf_counter() - t0)
        bn.append(F / float(np.median(best)))
    print(f"  relocalize_batch F = {F}, 5 iterations: Newton {bn[0]:.1f}, Gauss-Newton {bn[1]:.1f} relocalisations/s")
    kf.close()
    return one[1] < d21


if __name__ == "__main__":
    which = sys.argv[1:] or ["reloc:1024", "s1:512"]
    good = True
    for w in which:
        name, n = w.split(":")
        good = main(name, int(n)) and good
    if not good:
        print("DEFECT: one launch at F = 1 is not faster than the 21 dense launches")
    sys.exit(0 if good else 1)
