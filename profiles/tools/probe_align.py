"""Map alignment, measured on scene S1 at 512^3 after 30 tracked frames: the other map is this map merged into an
empty 512^3 instance under a whole-voxel shift, the start half a voxel and 0.5 degrees off the truth.  Reports
  - one pass of xs_tsdf_align_terms over this map's band index at N = 1, 8 and 32 transforms (hipEvent pairs, the 0.6 KB map upload per
    transform included), and beside it, on the same index, one pass of xs_tsdf_gauss_newton_terms_band at F = 1 (frame 30 at its own pose);
  - a full KinectFusion.align_map (10 iterations and the loss pass, the device drained first) by the host's clock, and where it ends.
Every figure is the median of 20 runs after a warm-up.  No time is a condition.  One process; every GPU step runs under its own time limit (a
watchdog that ends the process), and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_align.py > profiles/align_probe.txt"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_score_views import scene, step_limit  # noqa: E402


def main(n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    sh = importlib.import_module("x-slam_amd.sharded")
    import align_cases as ac
    from helpers import intr_of, tranc_dist
    from independent_cases import seeded_poses

    with step_limit(240, f"scene s1 {n}^3"):
        kf, prm, nmap = scene("s1", n)
    vs = float(np.float32(prm["tsdf_voxel_size"]))
    res = [n, n, n]
    with step_limit(120, "the other map"):
        other = pl.KinectFusion(prm)
        into = np.eye(4)
        into[:3, 3] = np.array([3, -2, 1]) * vs
        written = other.merge_map(kf, into)
    T_true = np.eye(4)
    T_true[:3, 3] = -into[:3, 3]
    T0 = ac.perturbed(T_true, res, vs)
    print(f"---- scene s1, {n}^3 against {n}^3, map of {nmap} frames, the other map {written} voxels, one MI355X")

    p, step = kf.volume_ptr("value")
    assert step == n * 4, "the probe reads the value array as the dense map"
    kf.rebuild_sign_map()                      # (volume_ptr("value") marked the volume written)
    gt = torch.as_tensor(sh._DevView(p, n * n * n, "<f4"), device="cuda")
    with step_limit(120, "index"):
        idx = capi.tsdf_band_build(gt, res)
    ov, ostep = other.volume_ptr("value")
    ow, _ = other.volume_ptr("weight")
    other.rebuild_sign_map()
    print(f"index: {idx.count} band voxels ({idx.count * 12 / 2**20:.1f} MiB of keys + values)")

    def timed(fn, reps=20):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms))

    ws = torch.zeros(capi.tsdf_align_workspace_bytes(32), dtype=torch.uint8, device="cuda")
    out = torch.zeros(29 * 32, dtype=torch.float64, device="cuda")
    one = pl.align_seeded_maps(T0, vs, vs)
    print("pass kernel time, median of 20 (min):")
    for N in (1, 8, 32):
        maps = np.repeat(one[None], N, axis=0)
        with step_limit(120, f"align pass N = {N}"):
            med, lo = timed(lambda: capi.tsdf_align_terms(idx, ov, ow, ostep, res, maps, 1, 1.0, ws, out))
        s = out[:29].cpu().numpy()
        print(f"  xs_tsdf_align_terms N = {N:2d}: {med * 1e3:8.1f} us per launch ({lo * 1e3:.1f}), {med * 1e3 / N:7.1f} us per transform; kept {int(s[28])} of {idx.count}")
    W, H = synth.WIDTH, synth.HEIGHT
    frame = torch.from_numpy(synth.s1_frame(nmap).view(np.int16)).cuda()
    scaled = torch.empty((H, W), dtype=torch.float32, device="cuda")
    capi.scale_depth(frame, W * 2, H, W, scaled, W * 4)
    R, t = seeded_poses(kf.camera2volume()[..., 0].astype(np.float64))
    bws = torch.zeros(capi.tsdf_band_workspace_bytes(1), dtype=torch.uint8, device="cuda")
    with step_limit(120, "Gauss-Newton band pass"):
        med, lo = timed(lambda: capi.tsdf_gauss_newton_terms_band([scaled], W * 4, H, W, intr_of(prm), vs, R[None], t[None], tranc_dist(prm), idx, bws, out))
    s = out[:29].cpu().numpy()
    print(f"  xs_tsdf_gauss_newton_terms_band F = 1 (the frame path's relocalisation pass, same index): {med * 1e3:8.1f} us ({lo * 1e3:.1f}); kept {int(s[28])}")
    del idx, gt

    with step_limit(300, "align_map"):
        ok, T, rep, hist = kf.align_map(other, T0)          # (builds the orchestrator's own index and workspace)
        secs = []
        for _ in range(20):
            t0 = time.perf_counter()
            ok, T, rep, hist = kf.align_map(other, T0)
            secs.append(time.perf_counter() - t0)
    print(f"align_map, 10 iterations + the loss pass, one start: {np.median(secs) * 1e3:.2f} ms (median of 20, host clock; min {min(secs) * 1e3:.2f}), "
          f"{np.median(secs) * 1e6 / rep['passes']:.0f} us per pass")
    print(f"  ok {ok}, loss {hist[0]:.3e} -> {hist[-1]:.3e}, kept {rep['count']} of {rep['band_voxels']}, "
          f"{ac.corner_displacement(T, T_true, res, vs) / vs:.2e} voxel edges from the truth at the worst corner "
          f"(the start: {ac.corner_displacement(T0, T_true, res, vs) / vs:.2f})")
    other.close()
    kf.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
