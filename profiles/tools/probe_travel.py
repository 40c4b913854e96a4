"""Travel field, path and voxel query over the reached set, measured on scene S1 at 512^3 after 30 tracked frames, on
the flood of profiles/tools/probe_reach.py (a body of 0.03 m on the R = 32 field, seeded 0.4 m down the optical axis).  Reports
  - xs_reach_flood's rounds on that input, next to them xs_travel_build's rounds, domain voxels, largest cost and time from the same seed at
    the full limit (the call synchronises after every batch of rounds; the time is the whole call's: fill, seeding, rounds, read-backs);
  - xs_travel_path for the reached voxel with the largest cost (one target): its length and the time;
  - xs_travel_query for 4096 voxels (the answering voxels of xs_reach_query for Halton candidates in a 0.3 m box round the last pose).
No time is a condition; the exit status is 1 only if two builds on the same inputs disagree.  One process; every GPU step runs under its own
time limit (a watchdog that ends the process), and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_travel.py > profiles/travel_probe.txt"""
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
    R, body = 32, 0.03
    rv = np.float32(body) / np.float32(vs)
    r2 = max(1, int(np.ceil(np.float32(rv * rv))))
    with step_limit(240, "grid, field, flood"):
        grid = torch.zeros(capi.view_grid_bytes(res), dtype=torch.uint8, device="cuda")
        capi.view_grid_build(pv, pw, step, res, grid)
        field = torch.zeros(capi.clearance_bytes(res) // 2, dtype=torch.int16, device="cuda")
        ws = torch.zeros(capi.clearance_workspace_bytes(res), dtype=torch.uint8, device="cuda")
        capi.clearance_build(grid, res, R, 1, ws, field)
        del ws
        reach = torch.zeros(capi.reach_bytes(res), dtype=torch.uint8, device="cuda")
        capi.reach_passable(grid, field, res, r2, reach)
        c2v = kf.camera2volume()[..., 0]
        start = torch.from_numpy(np.ascontiguousarray(c2v[:3, 3] + np.float32(0.4) * c2v[:3, 2], np.float32)).cuda()
        flag, c2 = torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int16, device="cuda")
        seed = torch.zeros(3, dtype=torch.int32, device="cuda")
        capi.reach_query(1, start, res, vs, reach, field, flag, c2, snap=16, over_passable=True, voxel=seed)
        torch.cuda.synchronize()
        seed_h = seed.cpu().numpy()
        flood_rounds = capi.reach_flood(grid, field, res, r2, seed_h[None], reach)
        out = torch.zeros(n ** 3, dtype=torch.uint8, device="cuda")
        capi.reach_expand(reach, res, out)
        reached = int(out.sum(dtype=torch.int64))
        del out
        print(f"body {body} m (r2 = {r2}) on the R = {R} field, seed {tuple(int(v) for v in seed_h)} (found: {int(flag.item())}): xs_reach_flood took {flood_rounds} rounds, "
              f"reached {reached} voxels")
    tbytes = capi.travel_bytes(res)
    print(f"travel field {tbytes / 2**20:.0f} MiB, workspace {capi.travel_workspace_bytes()} bytes")
    travel = torch.zeros(tbytes // 2, dtype=torch.int16, device="cuda")
    tws = torch.zeros(capi.travel_workspace_bytes(), dtype=torch.uint8, device="cuda")
    with step_limit(300, "travel build"):
        rounds = []
        ms = timed(torch, lambda: rounds.append(capi.travel_build(reach, res, seed_h[None], capi.TRAVEL_MAX, travel, tws)), reps=5)
        a = travel.clone()
        capi.travel_build(reach, res, seed_h[None], capi.TRAVEL_MAX, travel, tws)
        torch.cuda.synchronize()
        good = bool(torch.equal(a, travel))
        del a
        cost = travel.to(torch.int32) & 0xffff
        finite = cost != capi.TRAVEL_NONE
        nfinite = int(finite.sum())
        far = int(torch.where(finite, cost, torch.zeros_like(cost)).argmax())
        top = int(cost[far])
        del cost, finite
        tiles = (n // 8) ** 3
        print(f"xs_travel_build from that seed, limit {capi.TRAVEL_MAX}: {ms * 1e3:9.0f} us (median of 5, the whole call: fill, seeding, {sorted(set(rounds))} rounds of "
              f"{tiles} workgroups in batches of 8 with a read-back each); voxels with a cost {nfinite} (reached {reached}); largest cost {top} = "
              f"{top * vs / 3:.2f} m; two builds equal: {good}")
        good = good and nfinite == reached
    with step_limit(120, "path"):
        target = torch.tensor([far % n, far // n % n, far // (n * n)], dtype=torch.int32, device="cuda")
        capacity = top // 3 + 2
        path = torch.zeros(capacity * 3, dtype=torch.int32, device="cuda")
        length = torch.zeros(1, dtype=torch.int32, device="cuda")
        ms = timed(torch, lambda: capi.travel_path(1, target, res, reach, travel, capi.TRAVEL_MAX, capacity, path, length), reps=10)
        print(f"xs_travel_path, one target at cost {top}: {ms * 1e3:9.0f} us (median of 10); {int(length.item())} voxels")
    with step_limit(120, "query"):
        cands = pl.pose_candidates(kf.camera2volume(), 0.3, 0.3, 4096)
        pts = torch.from_numpy(np.ascontiguousarray(cands[:, :3, 3, 0], np.float32).reshape(-1)).cuda()
        flags, clear2 = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(4096, dtype=torch.int16, device="cuda")
        voxel = torch.zeros(3 * 4096, dtype=torch.int32, device="cuda")
        capi.reach_query(4096, pts, res, vs, reach, field, flags, clear2, snap=0, voxel=voxel)
        costs = torch.zeros(4096, dtype=torch.int16, device="cuda")
        ms = timed(torch, lambda: capi.travel_query(4096, voxel, res, travel, costs), reps=20)
        with_cost = int(((costs.to(torch.int32) & 0xffff) != capi.TRAVEL_NONE).sum())
        print(f"xs_travel_query, 4096 voxels: {ms * 1e3:7.1f} us (median of 20); with a cost: {with_cost} (reached by the flood: {int(flags.sum())})")
        good = good and with_cost == int(flags.sum())
    kf.close()
    return good


if __name__ == "__main__":
    which = sys.argv[1:] or ["s1:512"]
    good = True
    for w in which:
        name, n = w.split(":")
        good = main(name, int(n)) and good
    if not good:
        print("DEFECT: two builds disagree, or the voxels with a cost are not the reached ones")
    sys.exit(0 if good else 1)
