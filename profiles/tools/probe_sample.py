"""Sampling the map at the caller's points, measured on scene S1 at 512^3 after 30 tracked frames.  Alternating in one loop,
three warm-up rounds, then the median of 20 calls each between hipEvent pairs (the zeroing of the counts included; points and outputs stay on
the device):
  - xs_tsdf_sample_points at 2^20 points drawn uniformly in the volume, status and value alone;
  - the same points with the gradient as well (seven evaluations per point);
  - 2^20 points taken from export_point_cloud (repeated to 2^20; coherent, all near the surface), value alone and with the gradient;
  - xs_tsdf_sample_depth (frame_residuals' kernel) of a 640 x 480 frame at the tracked pose, status and value.
Points per second for each.  No time is a condition.  One process; every GPU step runs under its own time limit, and the first failure ends
the run.  Run in its own process:
    python profiles/tools/probe_sample.py > profiles/sample_probe.txt"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_score_views import step_limit  # noqa: E402


def main(n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    from helpers import intr_of
    nmap, N = 30, 1 << 20
    prm = synth.s1_params(n, seed=None)
    with step_limit(300, f"scene s1 {n}^3"):
        kf = pl.KinectFusion(prm)
        for k in range(nmap):
            frame = torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda()
            assert kf.process_frame(frame) == 1
        kf.synchronize()
    print(f"---- scene s1, {n}^3, map of {nmap} tracked frames, one MI355X, 2^20 points per launch")
    W, H = synth.WIDTH, synth.HEIGHT
    res, vs, k4 = [n, n, n], float(np.float32(prm["tsdf_voxel_size"])), intr_of(prm)
    (pv, step), (pw, _) = kf.volume_ptr("value"), kf.volume_ptr("weight")
    c2v = kf.camera2volume()[..., 0]
    with step_limit(300, "points and buffers"):
        rng = np.random.default_rng(0)
        uniform = torch.from_numpy((rng.uniform(0.0, n * vs, (N, 3))).astype(np.float32)).cuda()
        cloud = kf.export_point_cloud(max_buffer=4000000)[0]
        assert len(cloud) > 0
        surface = torch.from_numpy(np.ascontiguousarray(np.resize(cloud, (N, 3)))).cuda()
        status = torch.empty(N, dtype=torch.uint8, device="cuda")
        value = torch.empty(N, dtype=torch.float32, device="cuda")
        gradient = torch.empty((N, 3), dtype=torch.float32, device="cuda")
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def points(p, with_gradient):
        capi.sample_points(N, p, pv, pw, step, res, vs, status=status, value_out=value, gradient=gradient if with_gradient else None, counts=counts)

    def depth():
        capi.sample_depth(frame, W * 2, H, W, k4, c2v[:3, :3], c2v[:3, 3], pv, pw, step, res, vs, status=status, value_out=value, counts=counts)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    arms = {"uniform points, value": (N, lambda: points(uniform, False)), "uniform points, value + gradient": (N, lambda: points(uniform, True)),
            "surface points, value": (N, lambda: points(surface, False)), "surface points, value + gradient": (N, lambda: points(surface, True)),
            "depth frame 640 x 480, value": (H * W, depth)}
    ms = {a: [] for a in arms}
    with step_limit(600, "kernels"):
        for rep in range(23):
            for arm, (count, call) in arms.items():
                d = timed(call)
                if rep >= 3:
                    ms[arm].append(d)
                if rep == 22:
                    c = counts.cpu().numpy()
                    med = float(np.median(ms[arm]))
                    print(f"{arm:34s}: {med * 1e3:9.1f} us (median of 20; min {min(ms[arm]) * 1e3:.1f}); {count / (med * 1e-3) / 1e6:8.1f} Mpoints/s; "
                          f"outside, unseen, ok, no_depth = {c.tolist()}")
    print(f"the point cloud holds {len(cloud)} points")
    kf.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
