"""Fusing a point cloud into the map, measured on scene S1 at 512^3 after 30 tracked frames.  The points: 2^20 points of the
exported cloud (repeated to 2^20), the camera's position as origin.  Alternating in one loop, three warm-up rounds, then the median of 20 calls
each between hipEvent pairs (points, accumulator and counts stay on the device; the folds write a SCRATCH copy of the volume, so the map the
accumulates walk through stays what it was):
  - xs_tsdf_fuse_points_accumulate without and with carve: the scatter of 8-byte integer atomics, whose rate the micro-architecture notes do not
    give (they measure float dword atomics only);
  - xs_tsdf_fuse_points_fold over the whole volume after each of the two;
  - in the same loop xs_tsdf_sample_points (value and gradient) on the same points, and xs_tsdf_merge of the map into the scratch copy under the
    identity: the two yardsticks, a gather per point and a pass over every voxel.
Then a whole KinectFusion.fuse_points over the same device points by the host's clock: the median of five calls after one warm-up.
No time is a condition.  One process; every GPU step runs under its own time limit, and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_fuse.py > profiles/fuse_probe.txt"""
import importlib
import os
import sys
import time

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
    nmap, N = 30, 1 << 20
    prm = synth.s1_params(n, seed=None)
    with step_limit(300, f"scene s1 {n}^3"):
        kf = pl.KinectFusion(prm)
        for k in range(nmap):
            frame = torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda()
            assert kf.process_frame(frame) == 1
        kf.synchronize()
    print(f"---- scene s1, {n}^3, map of {nmap} tracked frames, one MI355X, 2^20 points per launch")
    res, vs, tranc = [n, n, n], float(np.float32(prm["tsdf_voxel_size"])), float(kf.tranc_dist())
    (pv, step), (pw, _), (pg, _) = kf.volume_ptr("value"), kf.volume_ptr("weight"), kf.volume_ptr("grad")
    with step_limit(300, "points and buffers"):
        cloud = kf.export_point_cloud(max_buffer=4000000)[0]
        assert len(cloud) > 0
        points = torch.from_numpy(np.ascontiguousarray(np.resize(cloud, (N, 3)))).cuda()
        origin = pl._real44(kf.camera2volume())[:3, 3].astype(np.float32)
        acc = torch.zeros(capi.fuse_accumulator_bytes(res) // 8, dtype=torch.int64, device="cuda")
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        written = torch.zeros(1, dtype=torch.int64, device="cuda")
        scratch = [torch.zeros(step * n * n, dtype=torch.uint8, device="cuda") for _ in range(3)]
        merge_ws = torch.zeros(capi.tsdf_merge_workspace_bytes(res, res), dtype=torch.uint8, device="cuda")
        status = torch.empty(N, dtype=torch.uint8, device="cuda")
        value = torch.empty(N, dtype=torch.float32, device="cuda")
        gradient = torch.empty((N, 3), dtype=torch.float32, device="cuda")
        identity = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)
        opts = {False: capi.fuse_opts(0.2, 5.0, False), True: capi.fuse_opts(0.2, 5.0, True)}
        torch.cuda.synchronize()

    def accumulate(carve):
        capi.fuse_points_accumulate(N, points, origin, res, vs, tranc, opts[carve], acc, counts)

    def fold():
        capi.fuse_points_fold(scratch[0], scratch[1], scratch[2], step, res, acc, 1, 100, written=written)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    arms = {"accumulate, band only": lambda: accumulate(False), "fold after the band-only accumulate": fold,
            "accumulate, carve": lambda: accumulate(True), "fold after the carving accumulate": fold,
            "sample_points value + gradient, the same points": lambda: capi.sample_points(N, points, pv, pw, step, res, vs, status=status, value_out=value, gradient=gradient),
            "merge of the map into the scratch copy, identity": lambda: capi.tsdf_merge(scratch[0], scratch[1], scratch[2], step, res, pv, pw, pg, step, res, identity,
                                                                                         workspace=merge_ws)}
    ms = {a: [] for a in arms}
    note = {}
    with step_limit(900, "kernels"):
        for rep in range(23):
            for arm, call in arms.items():
                counts.zero_()
                written.zero_()
                d = timed(call)
                if rep >= 3:
                    ms[arm].append(d)
                if arm.startswith("accumulate"):
                    c = counts.cpu().numpy()
                    note[arm] = f"; used {c[0]}, dropped {c[1]}, visits {c[2]}, outside {c[3]}", int(c[2])
                elif arm.startswith("fold"):
                    note[arm] = f"; voxels written {int(written.item())}", 0
        for arm in arms:
            med = float(np.median(ms[arm]))
            text, visits = note.get(arm, ("", 0))
            rate = f"; {visits / (med * 1e-3) / 1e9:.2f} G atomic adds/s, {8 * visits / (med * 1e-3) / 1e12:.3f} TB/s of added bytes" if visits else ""
            print(f"{arm:52s}: {med * 1e3:10.1f} us (median of 20; min {min(ms[arm]) * 1e3:.1f}){text}{rate}")
    assert not bool(acc.any())
    with step_limit(600, "fuse_points"):
        for carve in (False, True):
            wall = []
            for rep in range(6):
                t0 = time.perf_counter()
                got = kf.fuse_points(points, None, origin, carve=carve)
                if rep:
                    wall.append(time.perf_counter() - t0)
            print(f"fuse_points, 2^20 device points, carve {carve}: {np.median(wall) * 1e3:.2f} ms by the host's clock (median of 5; min {min(wall) * 1e3:.2f}), the "
                  f"device drain and the rebuild of the sign map and the model maps included; {got}")
    print(f"the point cloud holds {len(cloud)} points; accumulator {acc.numel() * 8 / 2 ** 30:.2f} GiB")
    kf.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
