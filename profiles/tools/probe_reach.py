"""Clearance field, flood and point query over the observation grid, measured on scene S1 at 512^3 after 30 tracked
frames.  Reports
  - the sizes of the field, its workspace and the reach buffer;
  - xs_clearance_build at R = 8 and R = 32, unknown_blocks = 1 (hipEvent pairs, median): the three launches together;
  - a flood from the camera for a body of 0.03 m: the start snapped over the passable words (xs_reach_passable + xs_reach_query; the
    camera centre, and a point 0.4 m down the optical axis inside the carved cone), then xs_reach_flood — rounds, reached voxels and time
    (the call synchronises after every batch of rounds; the time is the whole call's);
  - xs_reach_query for 4096 points (the centres of Halton candidates in a 0.3 m box round the last pose) at snap 0 and snap 4.
No time is a condition; the exit status is 1 only if two runs on the same inputs disagree.  One process; every GPU step runs under its own
time limit (a watchdog that ends the process), and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_reach.py > profiles/reach_probe.txt"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_newton import timed  # noqa: E402  (profiles/tools: hipEvent pairs, median after a warm-up)
from probe_score_views import scene, step_limit  # noqa: E402


def main(name, n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")

    with step_limit(240, f"scene {name} {n}^3"):
        kf, prm, nmap = scene(name, n)
    print(f"---- scene {name}, {n}^3, map of {nmap} frames, one MI355X")
    res = [n, n, n]
    vs = prm["tsdf_voxel_size"]
    pv, step = kf.volume_ptr("value")
    pw, _ = kf.volume_ptr("weight")
    good = True
    with step_limit(120, "grid build"):
        grid = torch.zeros(capi.view_grid_bytes(res), dtype=torch.uint8, device="cuda")
        capi.view_grid_build(pv, pw, step, res, grid)
        torch.cuda.synchronize()
    fbytes, wbytes, rbytes = capi.clearance_bytes(res), capi.clearance_workspace_bytes(res), capi.reach_bytes(res)
    print(f"field {fbytes / 2**20:.0f} MiB, workspace {wbytes / 2**20:.0f} MiB, reach buffer {rbytes / 2**20:.1f} MiB (observation grid {grid.numel() / 2**20:.1f} MiB)")
    field = torch.zeros(fbytes // 2, dtype=torch.int16, device="cuda")
    ws = torch.zeros(wbytes, dtype=torch.uint8, device="cuda")
    for R in (8, 32):
        with step_limit(240, f"clearance R = {R}"):
            ms = timed(torch, lambda: capi.clearance_build(grid, res, R, 1, ws, field), reps=10)
            a = field.clone()
            capi.clearance_build(grid, res, R, 1, ws, field)
            torch.cuda.synchronize()
            same = bool(torch.equal(a, field))
            good = good and same
            at_cap = int((field.to(torch.int32) & 0xffff).eq(R * R).sum())
            print(f"xs_clearance_build R = {R:2d}, unknown_blocks = 1: {ms * 1e3:9.0f} us (median of 10; three launches); voxels at the cap R^2: {at_cap}; "
                  f"two builds equal: {same}")
            del a
    # a body of 0.03 m (two voxels at this size), on the R = 32 field.  The depth range starts at 0.2 m, so the carved free space begins some
    # 13 voxels in front of the camera at a 15 mm voxel: the camera's own position is tried with the largest snap, and the flood then starts
    # 0.4 m down the optical axis, inside the carved cone.
    body = 0.03
    rv = np.float32(body) / np.float32(vs)
    r2 = max(1, int(np.ceil(np.float32(rv * rv))))
    reach = torch.zeros(rbytes, dtype=torch.uint8, device="cuda")
    with step_limit(240, "flood"):
        c2v = kf.camera2volume()[..., 0]
        flag, c2 = torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int16, device="cuda")
        seed = torch.zeros(3, dtype=torch.int32, device="cuda")
        capi.reach_passable(grid, field, res, r2, reach)
        for what, p in (("the camera centre", c2v[:3, 3]), ("0.4 m down the optical axis", c2v[:3, 3] + np.float32(0.4) * c2v[:3, 2])):
            start = torch.from_numpy(np.ascontiguousarray(p, np.float32)).cuda()
            capi.reach_query(1, start, res, vs, reach, field, flag, c2, snap=16, over_passable=True, voxel=seed)
            torch.cuda.synchronize()
            seed_h = seed.cpu().numpy()
            print(f"start at {what}, voxel {tuple(int(v) for v in np.floor(p / np.float32(vs)))}: nearest passable voxel within snap 16: "
                  f"{tuple(int(v) for v in seed_h) if int(flag.item()) else 'none'}")
        rounds = []
        ms = timed(torch, lambda: rounds.append(capi.reach_flood(grid, field, res, r2, seed_h[None], reach)), reps=5)
        a = reach[:rbytes - 256].clone()
        capi.reach_flood(grid, field, res, r2, seed_h[None], reach)
        same = bool(torch.equal(a, reach[:rbytes - 256]))
        good = good and same
        out = torch.zeros(n ** 3, dtype=torch.uint8, device="cuda")
        capi.reach_expand(reach, res, out)
        reached = int(out.sum(dtype=torch.int64))
        capi.reach_expand(reach, res, out, passable=True)
        passable = int(out.sum(dtype=torch.int64))
        del out, a
        print(f"xs_reach_flood for a body of {body} m (r2 = {r2}) from that voxel: {ms * 1e3:9.0f} us (median of 5, the whole call: passable words, seeding, "
              f"{sorted(set(rounds))} rounds in batches of 8 with a read-back each); reached {reached} of {passable} passable voxels; two floods equal: {same}")
    with step_limit(120, "query"):
        cands = pl.pose_candidates(kf.camera2volume(), 0.3, 0.3, 4096)
        pts = torch.from_numpy(np.ascontiguousarray(cands[:, :3, 3, 0], np.float32).reshape(-1)).cuda()
        flags, clear2 = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(4096, dtype=torch.int16, device="cuda")
        for snap in (0, 4):
            ms = timed(torch, lambda: capi.reach_query(4096, pts, res, vs, reach, field, flags, clear2, snap=snap), reps=20)
            print(f"xs_reach_query, 4096 points, snap {snap}: {ms * 1e3:7.1f} us (median of 20); answers 1: {int(flags.sum())}")
    kf.close()
    return good


if __name__ == "__main__":
    which = sys.argv[1:] or ["s1:512"]
    good = True
    for w in which:
        name, n = w.split(":")
        good = main(name, int(n)) and good
    if not good:
        print("DEFECT: two runs on the same inputs disagree")
    sys.exit(0 if good else 1)
