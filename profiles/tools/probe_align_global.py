"""Scoring map-to-map transforms and aligning with no guess, measured on scene S1 at 512^3 after 30 tracked frames:
the other map is this map merged into an empty 512^3 instance under a rotation of 10 degrees about the volume's centre plus a shift.  Reports
  - one launch of xs_tsdf_score_transforms over this map's band index at P = 64, 512 and 4096 transforms (align_search_free's candidates, the
    truth among them), strides 1 and 4: hipEvent pairs, the 48-byte map upload per transform included, as microseconds and as scored
    (entry, transform) pairs per second;
  - a whole KinectFusion.align_map_global at the defaults (the device drained first) by the host's clock, and where it ends, beside
    align_map started at the truth.
Every kernel figure is the median of 20 runs after a warm-up.  No time is a condition.  One process; every GPU step runs under its own time
limit (a watchdog that ends the process), and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_align_global.py > profiles/align_global_probe.txt"""
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
    sh = importlib.import_module("x-slam_amd.sharded")
    import align_cases as ac

    with step_limit(240, f"scene s1 {n}^3"):
        kf, prm, nmap = scene("s1", n)
    vs = float(np.float32(prm["tsdf_voxel_size"]))
    res = [n, n, n]
    c = 0.5 * n * vs * np.ones(3)
    T_true = np.eye(4)                         # this map's frame -> the other's
    T_true[:3, :3] = ac.rotation((0.5, -0.3, 1.0), np.radians(10.0))
    T_true[:3, 3] = c - T_true[:3, :3] @ c + np.array([0.23, -0.17, 0.11])
    with step_limit(120, "the other map"):
        other = pl.KinectFusion(prm)
        written = other.merge_map(kf, np.linalg.inv(T_true))     # the other map's voxels sample this map under T_true^-1
    print(f"---- scene s1, {n}^3 against {n}^3, map of {nmap} frames, the other map {written} voxels (10 degrees + a shift), one MI355X")

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
    c_this = pl.band_centroid(idx.keys_t[:idx.count].cpu().numpy(), vs)

    def timed(fn, reps=20):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms)), float(min(ms))

    ws = torch.zeros(capi.tsdf_score_transforms_workspace_bytes(4096), dtype=torch.uint8, device="cuda")
    out = torch.zeros(2 * 4096, dtype=torch.float64, device="cuda")
    Ts = pl.transform_candidates_free(4096, c_this, T_true[:3, :3] @ c_this + T_true[:3, 3], float(kf.tranc_dist()))
    Ts[0] = T_true
    xforms = np.stack([pl.merge_affine(T, vs, vs) for T in Ts])
    print("launch time, median of 20 (min):")
    for stride in (1, 4):
        scored = -(-idx.count // stride)
        for P in (64, 512, 4096):
            with step_limit(240, f"score P = {P} stride {stride}"):
                med, lo = timed(lambda: capi.tsdf_score_transforms(idx, stride, ov, ow, ostep, res, xforms[:P], 1, 1.0, ws, out))
            s = out[:2 * P].cpu().numpy().reshape(P, 2)
            print(f"  xs_tsdf_score_transforms P = {P:4d} stride {stride}: {med * 1e3:10.1f} us per launch ({lo * 1e3:.1f}), {med * 1e3 / P:7.2f} us per transform, "
                  f"{scored * P / (med * 1e-3):.3e} pairs/s; the truth keeps {int(s[0, 1])} of {scored}, {int((s[:, 1] > 0).sum())} transforms keep any")
    del idx, gt

    with step_limit(600, "align_map_global"):
        ok, T, rep = kf.align_map_global(other)         # (builds the orchestrator's own index and workspace)
        secs = []
        for _ in range(5):
            t0 = time.perf_counter()
            ok, T, rep = kf.align_map_global(other)
            secs.append(time.perf_counter() - t0)
    print(f"align_map_global at the defaults: {np.median(secs) * 1e3:.1f} ms (median of 5, host clock; min {min(secs) * 1e3:.1f}); "
          f"{rep['score_launches']} scoring launches of {rep['scored_entries']} entries, {rep['passes']} alignment passes")
    print(f"  ok {ok}, rank {rep['rank']} after the last round, kept {rep['count']} of {rep['band_voxels']}, loss {rep['loss']:.3e}, "
          f"S {rep['count'] - rep['sum_r2']:.1f}, {ac.corner_displacement(T, T_true, res, vs) / vs:.2e} voxel edges from the truth at the worst corner")
    with step_limit(120, "align_map from the truth"):
        r_ok, r_T, r_rep, _ = kf.align_map(other, T_true)
    print(f"  align_map started at the truth, for comparison: ok {r_ok}, kept {r_rep['count']}, loss {r_rep['loss']:.3e}, S {r_rep['count'] - r_rep['sum_r2']:.1f}, "
          f"ends {ac.corner_displacement(r_T, T_true, res, vs) / vs:.2e} voxel edges from the truth; the search's answer is "
          f"{ac.corner_displacement(T, r_T, res, vs) / vs:.2e} voxel edges from it")
    other.close()
    kf.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
