"""Registering a point cloud to the map, measured on scene S1 at 512^3 after 30 tracked frames.  Alternating in one loop,
three warm-up rounds, then the median of 20 calls each between hipEvent pairs (points, workspace and sums stay on the device):
  - xs_tsdf_register_terms, one pass of N = 1, 8 and 32 transforms over 2^20 points of the exported cloud (repeated to 2^20; coherent, all near
    the surface) and over 2^20 points drawn uniformly in the volume;
  - in the same loop xs_tsdf_sample_points with value and gradient on the same points: the yardstick.  A registration pass does the same seven
    evaluations per point and transform, and writes 29 doubles where that call writes seventeen bytes per point.
Then a whole KinectFusion.register_points of ten iterations (eleven launches and fetches) over the 2^20 surface points, displaced by 1 cm and
0.5 degrees, device points, by the host's clock: the median of five calls after one warm-up.
No time is a condition.  One process; every GPU step runs under its own time limit, and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_register.py > profiles/register_probe.txt"""
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
    import align_cases as ac
    nmap, N = 30, 1 << 20
    prm = synth.s1_params(n, seed=None)
    with step_limit(300, f"scene s1 {n}^3"):
        kf = pl.KinectFusion(prm)
        for k in range(nmap):
            frame = torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda()
            assert kf.process_frame(frame) == 1
        kf.synchronize()
    print(f"---- scene s1, {n}^3, map of {nmap} tracked frames, one MI355X, 2^20 points per launch")
    res, vs = [n, n, n], float(np.float32(prm["tsdf_voxel_size"]))
    (pv, step), (pw, _) = kf.volume_ptr("value"), kf.volume_ptr("weight")
    with step_limit(300, "points and buffers"):
        rng = np.random.default_rng(0)
        uniform = torch.from_numpy((rng.uniform(0.0, n * vs, (N, 3))).astype(np.float32)).cuda()
        cloud = kf.export_point_cloud(max_buffer=4000000)[0]
        assert len(cloud) > 0
        surface_host = np.ascontiguousarray(np.resize(cloud, (N, 3)))
        surface = torch.from_numpy(surface_host).cuda()
        status = torch.empty(N, dtype=torch.uint8, device="cuda")
        value = torch.empty(N, dtype=torch.float32, device="cuda")
        gradient = torch.empty((N, 3), dtype=torch.float32, device="cuda")
        ws = torch.zeros(capi.register_workspace_bytes(32), dtype=torch.uint8, device="cuda")
        sums = torch.zeros(32 * 29, dtype=torch.float64, device="cuda")
        # 32 transforms within 1 cm and 0.5 degrees of the identity: every one keeps about the points the identity keeps
        X = [np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], np.float32)]
        for k in range(31):
            T = ac.perturbed(np.eye(4), res, vs, shift_voxels=rng.uniform(-1, 1, 3) * 0.01 / vs, degrees=float(rng.uniform(0.05, 0.5)), axis=rng.normal(size=3))
            X.append(np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]).astype(np.float32))
        X = np.stack(X)
        torch.cuda.synchronize()

    def sample(p):
        capi.sample_points(N, p, pv, pw, step, res, vs, xform12=X[0], status=status, value_out=value, gradient=gradient)

    def terms(p, count):
        capi.register_terms(N, p, X[:count], pv, pw, step, res, vs, 1, 0.9, ws, sums)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    arms = {}
    for name, p in (("surface", surface), ("uniform", uniform)):
        arms[f"{name} points, sample_points value + gradient"] = (1, lambda p=p: sample(p))
        for count in (1, 8, 32):
            arms[f"{name} points, register_terms N = {count}"] = (count, lambda p=p, count=count: terms(p, count))
    ms = {a: [] for a in arms}
    with step_limit(600, "kernels"):
        for rep in range(23):
            for arm, (count, call) in arms.items():
                d = timed(call)
                if rep >= 3:
                    ms[arm].append(d)
                if rep == 22:
                    med = float(np.median(ms[arm]))
                    kept = "" if "sample_points" in arm else f"; kept by transform 0: {int(sums[28].item())}"
                    print(f"{arm:52s}: {med * 1e3:9.1f} us (median of 20; min {min(ms[arm]) * 1e3:.1f}); {med * 1e3 / count:9.1f} us per transform; "
                          f"{count * N / (med * 1e-3) / 1e6:8.1f} Mpoints/s{kept}")
    with step_limit(600, "register_points"):
        T_true = ac.perturbed(np.eye(4), res, vs, shift_voxels=np.array([0.6, -0.5, 0.62]) / np.linalg.norm([0.6, -0.5, 0.62]) * 0.01 / vs, degrees=0.5)
        inv = np.linalg.inv(T_true)
        moved = torch.from_numpy((surface_host.astype(np.float64) @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32)).cuda()
        wall = []
        for rep in range(6):
            t0 = time.perf_counter()
            ok, T, rep_ = kf.register_points(moved, iterations=10)
            if rep:
                wall.append(time.perf_counter() - t0)
        print(f"register_points, ten iterations, 2^20 device points 1 cm and 0.5 degrees off: {np.median(wall) * 1e3:.2f} ms by the host's clock (median of 5; min "
              f"{min(wall) * 1e3:.2f}); ok {ok}, passes {rep_['passes']}, kept {rep_['count']}, loss {rep_['loss_history'][0]:.3e} -> {rep_['loss']:.3e}, "
              f"corner distance from the truth {ac.corner_displacement(np.eye(4), T_true, res, vs):.3e} -> {ac.corner_displacement(T, T_true, res, vs):.3e} m")
    print(f"the point cloud holds {len(cloud)} points")
    kf.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
