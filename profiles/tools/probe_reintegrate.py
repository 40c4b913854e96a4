"""Signed re-integration, measured on scene S1 at 512^3 after 30 tracked frames.  Alternating in one loop, three
warm-up rounds, then the median of 20 calls each between hipEvent pairs:
  - one xs_tsdf_reintegrate launch of [-1, +1] (frame 25 taken out and put back at its own pose);
  - one launch of eight ops (frames 22, 24, 26, 28, each taken out and put back);
  - beside each the yardstick: the same number of xs_integrate_scaled_ex calls with XS_INTEGRATE_NO_TILES for the same frames and poses — the
    integrate kernels' exact per-voxel walk, brick list and all, which is what fusing those frames costs without this kernel.
Every arm works on device copies of the map that are restored outside the timed spans.  Then, by a host clock around calls that end in a
synchronise, the median of 5 after one warm-up: KinectFusion.reintegrate (drain, scale, one launch, sign map, point cloud, model maps).
Then what refine_frame is for, at 64^3 and 256^3 on scene S3 tracked normally, as tests/test_reintegrate_pipeline_gpu.py sets it up: frame 3 is
moved to a pose off by 1 cm and 0.5 degrees; how far from the true pose refine_frame ends, next to relocalize from the same start on the map
that still holds the frame.  No time is a condition; the exit status is 1 only if the [-1, +1] launch with the cull and without it disagree in a
bit or a count.  One process; every GPU step runs under its own time limit, and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_reintegrate.py > profiles/reintegrate_probe.txt"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_score_views import step_limit  # noqa: E402

NO_TILES = 32   # XS_INTEGRATE_NO_TILES


def v2c_of(c2v):
    m = np.linalg.inv(c2v[..., 0].astype(np.complex128) + 1j * c2v[..., 1])
    R, t = np.zeros((3, 3, 2), np.float32), np.zeros((3, 2), np.float32)
    R[..., 0], R[..., 1], t[..., 0], t[..., 1] = m[:3, :3].real, m[:3, :3].imag, m[:3, 3].real, m[:3, 3].imag
    return R, t


def kernels(n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    from helpers import intr_of, tranc_dist
    nmap = 30
    prm = synth.s1_params(n, seed=None)
    with step_limit(300, f"scene s1 {n}^3"):
        kf = pl.KinectFusion(prm)
        frames, c2v = [], []
        for k in range(nmap):
            frames.append(torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda())
            assert kf.process_frame(frames[k]) == 1
            c2v.append(kf.camera2volume().copy())
        kf.synchronize()
    print(f"---- scene s1, {n}^3, map of {nmap} tracked frames, one MI355X")
    W, H = synth.WIDTH, synth.HEIGHT
    res, vs, td, k4, mw = [n, n, n], float(np.float32(prm["tsdf_voxel_size"])), tranc_dist(prm), intr_of(prm), int(prm["max_integration_weight"])
    step = n * 4
    with step_limit(120, "copies and images"):
        orig = [torch.from_numpy(a.reshape(n * n, n)).cuda() for a in kf.volume()]      # the map, through the host: value, weight, grad
        work = [t.clone() for t in orig]
        scaled = {}
        for k in (22, 24, 25, 26, 28):
            scaled[k] = torch.empty((H, W), dtype=torch.float32, device="cuda")
            capi.scale_depth(frames[k], W * 2, H, W, scaled[k], W * 4)
        ws = torch.zeros(capi.integrate_workspace_bytes(res), dtype=torch.uint8, device="cuda")
        counts = torch.zeros(4, dtype=torch.int64, device="cuda")
        updated = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def restore():
        for w, o in zip(work, orig):
            w.copy_(o)

    def ops_of(ks):
        out = []
        for k in ks:
            R, t = v2c_of(c2v[k])
            out += [(-1, scaled[k], R, t), (1, scaled[k], R, t)]
        return out

    def reintegrate(ops, flags=0):
        capi.tsdf_reintegrate(ops, W * 4, H, W, k4, mw, res, vs, td, work[0], work[1], work[2], step, counts, flags=flags)

    def integrate(ks, twice=True):
        for k in ks:
            R, t = v2c_of(c2v[k])
            for _ in range(2 if twice else 1):
                capi.integrate_scaled_ex(scaled[k], W * 4, H, W, k4, mw, res, vs, R, t, td, work[0], work[1], work[2], step, NO_TILES, updated=updated, workspace=ws)

    arms = {"reintegrate [-1, +1]": lambda: reintegrate(ops_of([25])), "integrate x 2, exact walk": lambda: integrate([25]),
            "reintegrate, 8 ops": lambda: reintegrate(ops_of([22, 24, 26, 28])), "integrate x 8, exact walk": lambda: integrate([22, 24, 26, 28])}
    ms = {a: [] for a in arms}
    with step_limit(420, "kernels"):
        for rep in range(23):
            for arm, call in arms.items():
                restore()
                counts.zero_()
                t = timed(call)
                if rep >= 3:
                    ms[arm].append(t)
                if rep == 22:
                    print(f"{arm:28s}: {np.median(ms[arm]) * 1e3:9.1f} us (median of 20; min {min(ms[arm]) * 1e3:.1f})"
                          + (f"; counts removed/added/emptied/orphaned {[int(c) for c in counts.cpu().numpy()]}" if arm.startswith("reint") else ""))
    r2, i2, r8, i8 = (np.median(ms[a]) for a in arms)
    print(f"[-1, +1] in one launch / two exact walks = {r2 / i2:.2f}; eight ops in one launch / eight exact walks = {r8 / i8:.2f}; "
          f"eight ops / [-1, +1] = {r8 / r2:.2f}; per op {r2 / 2 * 1e3:.1f} us and {r8 / 8 * 1e3:.1f} us")
    with step_limit(120, "cull against no cull"):
        outs = []
        for flags in (0, capi.REINTEGRATE_NO_CULL):
            restore()
            counts.zero_()
            t = timed(lambda: reintegrate(ops_of([25]), flags))
            outs.append(([w.clone() for w in work], [int(c) for c in counts.cpu().numpy()], t))
        same = outs[0][1] == outs[1][1] and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs[0][0], outs[1][0]))
        changed = sum(int((a.view(torch.int32) != o.view(torch.int32)).sum().item()) for a, o in zip(outs[0][0], orig))
        print(f"[-1, +1] without the cull: {outs[1][2] * 1e3:.1f} us (one call); equal to the culled launch: {same}; words that differ from the map before: {changed}")
        del outs
    with step_limit(120, "the orchestrator's call"):
        ts = []
        for rep in range(6):
            t0 = time.perf_counter()
            c = kf.reintegrate(frames[25], c2v[25], c2v[25])
            ts.append(time.perf_counter() - t0)
        print(f"KinectFusion.reintegrate (drain, scale, one launch, sign map, point cloud, model maps): {np.median(ts[1:]) * 1e3:.2f} ms (host clock, median of 5); {c}")
    kf.close()
    return same


def refine(n):
    import torch
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    import test_reintegrate_pipeline_gpu as tp
    prm = synth.s1_params(n)
    with step_limit(240, f"refine_frame at {n}^3"):
        frames = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(tp.FRAMES)]
        kf = pl.KinectFusion(prm)
        tracked = []
        for k in range(tp.FRAMES):
            assert kf.process_frame(frames[k]) == 1
            tracked.append(kf.camera2volume().copy())
        w2v = np.eye(4)
        w2v[:3, 3] = [prm["init_x"], prm["init_y"], prm["init_z"]]
        truth = w2v @ synth.s1_pose(tp.OUT)
        off = tracked[tp.OUT].copy()
        moved = tp.wrong(tracked[tp.OUT][..., 0].astype(np.float64) + 1j * tracked[tp.OUT][..., 1])
        off[..., 0], off[..., 1] = moved.real, moved.imag
        kf.reintegrate(frames[tp.OUT], tracked[tp.OUT], off)
        plain = kf.relocalize(frames[tp.OUT], off)
        ok, refined, hist, counts = kf.refine_frame(frames[tp.OUT], off)
        fmt = lambda d: f"{d[1] * 1e3:.2f} mm, {np.degrees(d[2]):.3f} deg"
        print(f"---- scene s3, {n}^3, six tracked frames; frame {tp.OUT} fused 1 cm and 0.5 degrees off its tracked pose; distances to the true pose:")
        print(f"the tracked pose {fmt(tp.pose_distance(tracked[tp.OUT], truth))}; the start {fmt(tp.pose_distance(off, truth))}; "
              f"refine_frame (ok {ok}) {fmt(tp.pose_distance(refined, truth))}; relocalize on the unmodified map (ok {plain[0]}) {fmt(tp.pose_distance(plain[1], truth))}; "
              f"loss {hist[0]:.3e} -> {hist[-1]:.3e}; {counts}")
        kf.close()


if __name__ == "__main__":
    good = kernels(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
    for size in (64, 256):
        refine(size)
    if not good:
        print("DEFECT: the cull changed the result")
    sys.exit(0 if good else 1)
