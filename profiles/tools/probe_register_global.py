"""Scoring many transforms of a point cloud and registering with no starting guess, measured on scene S1 at 512^3 after
30 tracked frames, over 2^20 points of the exported cloud (repeated to 2^20) handed over moved by a rotation of 100 degrees about an axis through
the volume's centre plus a shift.  The 4096 transforms are the search's own round 0: xs_host_align_search_free from the moved cloud's centroid to
the exported cloud's (which stands in for the map's band centroid here; the timing does not depend on it), box 3 voxels.
Alternating in one loop, one warm-up round, then the median of 5 rounds each between hipEvent pairs (points, workspace and sums stay on the device):
  (a) xs_tsdf_score_points: ONE launch of 4096 transforms, at stride 1 and at stride 4;
  (b) the only way to the same numbers before this call existed: 128 launches of xs_tsdf_register_terms with 32 transforms each, over all 2^20
      points (slot 27 and 28 of its 29 sums are sum r^2 and the count, behind a gradient gate of six more samples per point).
Then (c) a whole KinectFusion.register_points_global at its defaults (2048 candidates, stride 4, keep 8, 2 rounds, ten iterations from eight
starts over all 2^20 points), device points, by the host's clock: the median of 3 calls after one warm-up.
No time is a condition.  One process; every GPU step runs under its own time limit, and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_register_global.py > profiles/register_global_probe.txt"""
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
    nmap, N, P = 30, 1 << 20, 4096
    prm = synth.s1_params(n, seed=None)
    with step_limit(300, f"scene s1 {n}^3"):
        kf = pl.KinectFusion(prm)
        for k in range(nmap):
            frame = torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda()
            assert kf.process_frame(frame) == 1
        kf.synchronize()
    print(f"---- scene s1, {n}^3, map of {nmap} tracked frames, one MI355X, 2^20 points, {P} transforms")
    res, vs = [n, n, n], float(np.float32(prm["tsdf_voxel_size"]))
    (pv, step), (pw, _) = kf.volume_ptr("value"), kf.volume_ptr("weight")
    with step_limit(300, "points and buffers"):
        cloud = kf.export_point_cloud(max_buffer=4000000)[0]
        assert len(cloud) > 0
        surface = np.ascontiguousarray(np.resize(cloud, (N, 3))).astype(np.float64)
        c = 0.5 * n * vs * np.ones(3)
        T_true = np.eye(4)                                   # cloud frame -> volume frame
        T_true[:3, :3] = ac.rotation((0.5, -0.3, 1.0), np.radians(100.0))
        T_true[:3, 3] = c - T_true[:3, :3] @ c + np.array([0.23, -0.17, 0.11])
        inv = np.linalg.inv(T_true)
        moved_host = np.ascontiguousarray((surface @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
        moved = torch.from_numpy(moved_host).cuda()
        Ts = pl.transform_candidates_free(P, pl.points_centroid(moved_host, 4), surface.mean(axis=0), 3 * vs)
        X = np.stack([np.concatenate([T[:3, :3].reshape(-1), T[:3, 3]]) for T in Ts]).astype(np.float32)
        ws_score = torch.zeros(capi.tsdf_score_points_workspace_bytes(P), dtype=torch.uint8, device="cuda")
        pairs = torch.zeros(P * 2, dtype=torch.float64, device="cuda")
        ws_terms = torch.zeros(capi.register_workspace_bytes(32), dtype=torch.uint8, device="cuda")
        sums = torch.zeros(P * 29, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()

    def score(stride):
        capi.tsdf_score_points(N, moved, X, pv, pw, step, res, vs, 1, 0.9, ws_score, pairs, stride=stride)

    def terms():
        for g in range(P // 32):
            capi.register_terms(N, moved, X[32 * g:32 * g + 32], pv, pw, step, res, vs, 1, 0.9, ws_terms, sums[29 * 32 * g:])

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    arms = {"(a) score_points, 1 launch, stride 1": (N, lambda: score(1)), "(a) score_points, 1 launch, stride 4": (N // 4, lambda: score(4)),
            "(b) register_terms, 128 launches of 32": (N, terms)}
    ms = {a: [] for a in arms}
    kept = {}
    with step_limit(900, "kernels"):
        for rep in range(6):
            for arm, (scored, call) in arms.items():
                d = timed(call)
                if rep >= 1:
                    ms[arm].append(d)
                if rep == 5:
                    out = sums.cpu().numpy().reshape(P, 29)[:, 27:29] if arm.startswith("(b)") else pairs.cpu().numpy().reshape(P, 2)
                    kept[arm] = out.copy()
                    med = float(np.median(ms[arm]))
                    print(f"{arm:42s}: {med:10.2f} ms (median of 5; min {min(ms[arm]):.2f}); {med * 1e6 / (P * scored):7.3f} ns per point-transform pair; "
                          f"{P * scored / (med * 1e-3) / 1e9:8.2f} G pairs/s; kept per transform: mean {out[:, 1].mean():.0f}, max {out[:, 1].max():.0f}")
    a1, b = kept["(a) score_points, 1 launch, stride 1"], kept["(b) register_terms, 128 launches of 32"]
    ta, tb = float(np.median(ms["(a) score_points, 1 launch, stride 1"])), float(np.median(ms["(b) register_terms, 128 launches of 32"]))
    print(f"(b) / (a) at stride 1, per point-transform pair: {tb / ta:.2f}; transforms whose count (a) >= count (b): {(a1[:, 1] >= b[:, 1]).sum()} of {P} "
          f"(no gradient gate in (a)); the same best transform by S: {int(np.argmax(a1[:, 1] - a1[:, 0])) == int(np.argmax(b[:, 1] - b[:, 0]))}")
    with step_limit(900, "register_points_global"):
        wall = []
        for rep in range(4):
            t0 = time.perf_counter()
            ok, T, rep_ = kf.register_points_global(moved)
            if rep:
                wall.append(time.perf_counter() - t0)
        print(f"(c) register_points_global at the defaults, 2^20 device points: {np.median(wall) * 1e3:.1f} ms by the host's clock (median of 3; min {min(wall) * 1e3:.1f}); "
              f"ok {ok}, {rep_}, corner distance from the truth {ac.corner_displacement(T, T_true, res, vs):.3e} m")
        t0 = time.perf_counter()
        ok1, T1, rep1 = kf.register_points(moved, T_true, iterations=10)
        print(f"    register_points from the truth itself, ten iterations: {(time.perf_counter() - t0) * 1e3:.1f} ms; ok {ok1}, count {rep1['count']}, sum r^2 {rep1['sum_r2']:.4f}, "
              f"{ac.corner_displacement(T, T1, res, vs):.3e} m from the search's result")
    print(f"the point cloud holds {len(cloud)} points")
    kf.close()


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
