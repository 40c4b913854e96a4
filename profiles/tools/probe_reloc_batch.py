"""Batched relocalisation over the band index on bench.py's reloc scene: scene S3 with 7-Scenes intrinsics at
1024^3, a map of four frames, query frames 4 .. 4 + F - 1 from bench.py's perturbed starts (0.3 deg, ~1 cm).  Reports
  - the index build (two walks of the slab + the host's scan) and its size, and how evenly the band falls on the wave segments (a pass is
    as long as its busiest wave's segment);
  - one pass's kernel time (hipEvent pairs, median of 20) of the dense six-pose kernel and of the band kernel at F = 1, 4, 16;
  - relocalisations/s of relocalize_batch(F = 16) against a loop of relocalize calls (5 iterations + the final loss pass each).
Run in its own process:
    python profiles/tools/probe_reloc_batch.py [n] > profiles/reloc_batch_probe.txt"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    from helpers import intr_of, tranc_dist
    from independent_cases import seeded_poses

    nmap, F = 4, 16
    gtp = np.zeros((nmap, 4, 4, 2), np.float32)
    for k in range(nmap):
        gtp[k, ..., 0] = synth.s1_pose(k)
    prm = dict(synth.s1_params(n, seed=None), flag_use_gtPose=True, **synth.SEVEN_SCENES)   # bench.py reloc_workload's setup
    s3 = lambda k: synth.s3_frame(k, **synth.SEVEN_SCENES)
    kf = pl.KinectFusion(prm, gt_poses=gtp)
    for k in range(nmap):
        assert kf.process_frame(torch.from_numpy(s3(k).view(np.int16)).cuda()) == 1
    kf.synchronize()
    frames = [torch.from_numpy(s3(nmap + k).view(np.int16)).cuda() for k in range(F)]
    w2v = np.eye(4); w2v[:3, 3] = [prm["init_x"], prm["init_y"], prm["init_z"]]
    off = np.eye(4)
    a = np.radians(0.3)
    off[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    off[:3, 3] = [0.006, -0.005, 0.006]
    starts = [synth.cmat(w2v @ synth.s1_pose(nmap + k) @ off) for k in range(F)]
    W, H = synth.WIDTH, synth.HEIGHT
    print(f"scene S3, 7-Scenes intrinsics, {n}^3, map of {nmap} frames, {F} query frames, one MI355X")

    # ---- the index, built through the C ABI on the orchestrator's own value array (dense rows at this size)
    p, step = kf.volume_ptr("value")
    assert step == n * 4, "the probe reads the value array as the dense map"
    sh = importlib.import_module("x-slam_amd.sharded")
    gt = torch.as_tensor(sh._DevView(p, n * n * n, "<f4"), device="cuda")
    res = [n, n, n]
    times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        idx = capi.tsdf_band_build(gt, res)          # (count walk + fill walk: the probe's convenience builds twice over; the orchestrator
        torch.cuda.synchronize()                     #  builds once when its arrays are large enough — see the orchestrator line below)
        times.append((time.perf_counter() - t0) * 1e3)
    segs = idx.segs_t[:8 * idx.nblocks].cpu().numpy()
    cnt = segs[4 * idx.nblocks:]
    print(f"index: {idx.count} band voxels ({idx.count * 12 / 2**20:.1f} MiB of keys + values) in {idx.nblocks} workgroups x 4 wave segments")
    print(f"index build through capi (count-only call + count-and-fill call): {min(times):.1f} ms (best of 3)")
    print(f"wave segments: mean {cnt.mean():.0f}, max {cnt.max()} voxels ({cnt.max() / max(cnt.mean(), 1):.1f} x the mean), "
          f"{(cnt == 0).mean() * 100:.0f} % empty")

    # ---- one pass's kernel time
    k4, vs, trunc = intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm)
    scaled = [torch.empty((H, W), dtype=torch.float32, device="cuda") for _ in range(F)]
    for f in range(F):
        capi.scale_depth(frames[f], W * 2, H, W, scaled[f], W * 4)
    poses = [seeded_poses(s[..., 0].astype(np.float64)) for s in starts]
    ws = torch.zeros(capi.tsdf_reduce_workspace_bytes(), dtype=torch.uint8, device="cuda")
    bws = torch.zeros(capi.tsdf_band_workspace_bytes(capi.BAND_MAX_FRAMES), dtype=torch.uint8, device="cuda")
    out = torch.zeros(29 * capi.BAND_MAX_FRAMES, dtype=torch.float64, device="cuda")

    def timed(fn, reps=20):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    dense = timed(lambda: capi.tsdf_gauss_newton_terms(scaled[0], W * 4, H, W, k4, res, vs, poses[0][0], poses[0][1], trunc, gt, ws, out))
    print(f"pass kernel time, median of 20 (hipEvent pairs; band passes include the 0.6 KB pose upload per frame):")
    print(f"  dense six-pose pass (xs_tsdf_gauss_newton_terms), one frame: {dense * 1e3:.0f} us")
    for nf in (1, 4, 16):
        R, t = np.stack([poses[f][0] for f in range(nf)]), np.stack([poses[f][1] for f in range(nf)])
        ms = timed(lambda: capi.tsdf_gauss_newton_terms_band(scaled[:nf], W * 4, H, W, k4, vs, R, t, trunc, idx, bws, out))
        print(f"  band pass F = {nf:2d}: {ms * 1e3:.0f} us per launch, {ms * 1e3 / nf:.1f} us per frame-pass")
    del idx, gt

    # ---- relocalisations / s, the orchestrator's paths (5 iterations + final loss pass)
    kf.relocalize_batch(frames, np.stack(starts), iterations=5)          # (builds the orchestrator's index)
    torch.cuda.synchronize()
    gen_t0 = time.perf_counter()
    kf.rebuild_sign_map()                                                # (marks the volume written: the next batch rebuilds its index)
    kf.relocalize_batch(frames[:1], np.stack(starts[:1]), iterations=0)
    gen_ms = (time.perf_counter() - gen_t0) * 1e3
    print(f"orchestrator: index of {kf.relocalization_index_voxels()} voxels rebuilt + one loss pass: {gen_ms:.1f} ms")

    def loop():
        for f in range(F):
            ok, _, _ = kf.relocalize(frames[f], starts[f], iterations=5)
            assert ok

    def batch():
        ok, _, _ = kf.relocalize_batch(frames, np.stack(starts), iterations=5)
        assert ok.all()

    for name, fn in (("loop of relocalize", loop), ("relocalize_batch F = 16", batch)):
        fn()
        best = []
        for _ in range(5):
            t0 = time.perf_counter(); fn(); best.append(time.perf_counter() - t0)
        print(f"{name:26s}: {F / np.median(best):7.1f} relocalisations/s (median of 5 runs of {F} frames)")
    kf.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1024)
