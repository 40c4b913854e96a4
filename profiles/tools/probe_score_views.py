"""Scoring candidate views against the map in one launch, measured on
  - scene S1 at 512^3 after 30 tracked frames;
  - bench.py's reloc scene: S3 with 7-Scenes intrinsics at 1024^3, a map of four frames.
Reports per scene
  - the observation grid's size, the time of xs_view_grid_build (hipEvent pairs, median) and that time as a fraction of what 8 TB/s would
    need for the 8 bytes per voxel the build reads;
  - one launch of xs_score_views at P = 1, 64 and 4096 Halton candidates in a 0.3 m / 0.3 rad box round the last pose, the 80 x 60 lattice,
    depths 0.2 .. 5.0 in steps of a voxel: time (the pose upload and the zeroing of the counts included), nominal samples per second (P x
    rays x samples per ray) and the samples that fell into the volume;
  - FOR SCALE ONLY the time of P launches of xs_raycast at 640 x 480 at the same poses — the only way to look at a hypothetical view
    without this kernel; it answers another question (a vertex map, not counts of unknown space), so no ratio is formed.
No time is a condition; the exit status is 1 only if two launches disagree.  One process; every GPU step runs under its own time limit
(a watchdog that ends the process), and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_score_views.py > profiles/score_views_probe.txt"""
import contextlib
import faulthandler
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_newton import timed  # noqa: E402  (profiles/tools: hipEvent pairs, median after a warm-up)


@contextlib.contextmanager
def step_limit(seconds, what):
    """The step's own time limit: the process is ended (with the stacks on stderr) if the block has not finished by then, also when the main
    thread is blocked inside the runtime."""
    print(f"[step: {what}, limit {seconds} s]", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def scene(name, n):
    import torch
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    if name == "reloc":     # bench.py reloc_workload's setup
        nmap = 4
        gtp = np.zeros((nmap, 4, 4, 2), np.float32)
        for k in range(nmap):
            gtp[k, ..., 0] = synth.s1_pose(k)
        prm = dict(synth.s1_params(n, seed=None), flag_use_gtPose=True, **synth.SEVEN_SCENES)
        frame = lambda k: synth.s3_frame(k, **synth.SEVEN_SCENES)
        kf = pl.KinectFusion(prm, gt_poses=gtp)
    else:
        nmap = 30
        prm = synth.s1_params(n, seed=None)
        frame = synth.s1_frame
        kf = pl.KinectFusion(prm)
    for k in range(nmap):
        assert kf.process_frame(torch.from_numpy(frame(k).view(np.int16)).cuda()) == 1
    kf.synchronize()
    return kf, prm, nmap


def main(name, n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    from helpers import intr_of, tranc_dist

    with step_limit(240, f"scene {name} {n}^3"):
        kf, prm, nmap = scene(name, n)
    W, H = synth.WIDTH, synth.HEIGHT
    print(f"---- scene {name}, {n}^3, map of {nmap} frames, one MI355X")
    res = [n, n, n]
    pv, step = kf.volume_ptr("value")
    pw, wstep = kf.volume_ptr("weight")
    pg, _ = kf.volume_ptr("grad")
    assert step == wstep
    good = True

    with step_limit(120, "grid build"):
        gbytes = capi.view_grid_bytes(res)
        grid = torch.zeros(gbytes, dtype=torch.uint8, device="cuda")
        ms = timed(torch, lambda: capi.view_grid_build(pv, pw, step, res, grid), reps=10)
        states = torch.zeros(n * n * n, dtype=torch.uint8, device="cuda")
        capi.view_grid_expand(grid, res, states)
        hist = torch.bincount(states.to(torch.int64), minlength=3).cpu().numpy()
        del states
        floor_ms = 8.0 * n ** 3 / 8e12 * 1e3
        print(f"observation grid: {gbytes / 2**20:.1f} MiB (volumes: {8 * n**3 / 2**20:.0f} MiB of value + weight); voxels unknown / free / occupied "
              f"{hist[0]} / {hist[1]} / {hist[2]}")
        print(f"xs_view_grid_build: {ms * 1e3:.0f} us (median of 10); 8 B/voxel at 8 TB/s would take {floor_ms * 1e3:.0f} us: {floor_ms / ms:.2f} of that rate")

    k4, vs = intr_of(prm), prm["tsdf_voxel_size"]
    cands = pl.pose_candidates(kf.camera2volume(), 0.3, 0.3, capi.VIEW_MAX_POSES)
    R, t = np.ascontiguousarray(cands[:, :3, :3, 0]), np.ascontiguousarray(cands[:, :3, 3, 0])
    samples = 0
    while np.float32(0.2) + np.float32(samples) * np.float32(vs) < np.float32(5.0):
        samples += 1
    out = torch.zeros(4 * capi.VIEW_MAX_POSES, dtype=torch.int32, device="cuda")
    vm = torch.zeros((3 * H, W, 2), dtype=torch.float32, device="cuda")
    nm = torch.zeros((3 * H, W, 2), dtype=torch.float32, device="cuda")
    rws = torch.zeros(H * W, dtype=torch.float32, device="cuda")
    eye, zero = synth.cmat(np.eye(3)), synth.cmat(np.zeros(3))
    print(f"one launch of xs_score_views, 80 x 60 rays x {samples} samples per ray (hipEvent pairs; pose upload and zeroing of the counts included):")
    for P in (1, 64, 4096):
        with step_limit(120, f"score P = {P}"):
            one = timed(torch, lambda: capi.score_views(R[:P], t[:P], k4, H, W, res, vs, grid, out), reps=20)
            torch.cuda.synchronize()
            a = out[:4 * P].cpu().numpy().view(np.uint32).reshape(P, 4).copy()
            capi.score_views(R[:P], t[:P], k4, H, W, res, vs, grid, out)
            torch.cuda.synchronize()
            same = bool(np.array_equal(a, out[:4 * P].cpu().numpy().view(np.uint32).reshape(P, 4)))
            good = good and same
            nominal = P * 4800 * samples
            inside = int(a[:, :3].astype(np.int64).sum())
            print(f"  P = {P:4d}: {one * 1e3:8.0f} us (median of 20; {one * 1e3 / P:7.2f} us per pose); {nominal / (one * 1e-3):.3g} nominal samples/s, "
                  f"{inside} samples inside the volume ({inside / (one * 1e-3):.3g} /s); two launches equal: {same}; poses with hits >= 1200: "
                  f"{int((a[:, 2] >= 1200).sum())}, largest unknown count {int(a[:, 0].max())}")
        with step_limit(240, f"raycast x {P}"):
            def casts():
                for q in range(P):
                    capi.raycast(k4, synth.cmat(R[q]), synth.cmat(t[q]), eye, zero, tranc_dist(prm), res, vs, pv, pg, step, vm, nm, W * 8, H, W, workspace=rws)
            reps = 5 if P <= 64 else 1
            d = timed(torch, casts, reps=reps)
            print(f"            for scale: {P} launches of xs_raycast at 640 x 480 at the same poses {d * 1e3:9.0f} us "
                  f"({'median of 5' if reps > 1 else 'one run after a warm-up'}; vertex and normal maps, not counts)")
    kf.close()
    return good


if __name__ == "__main__":
    which = sys.argv[1:] or ["s1:512", "reloc:1024"]
    good = True
    for w in which:
        name, n = w.split(":")
        good = main(name, int(n)) and good
    if not good:
        print("DEFECT: two launches on the same inputs disagree")
    sys.exit(0 if good else 1)
