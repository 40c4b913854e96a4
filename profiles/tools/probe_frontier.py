"""Frontier mask, cluster labels and cluster records, measured on scene S1 at 512^3 after 30 tracked frames with
hipEvent pairs.  Reports
  - xs_frontier_mask: the time of the one launch and the number of frontier voxels;
  - xs_frontier_label at cell 0, 32 and 64: the whole call's time (seeding, rounds in batches of 8 with a read-back each) and its rounds;
  - xs_frontier_clusters on each labelling: the whole call's time (root compaction, the host's sort, accumulation) and the cluster count.
No time is a condition; the exit status is 1 only if two runs on the same inputs disagree.  One process; every GPU step runs under its own
time limit (a watchdog that ends the process), and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_frontier.py > profiles/frontier_probe.txt"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_newton import timed  # noqa: E402  (profiles/tools: hipEvent pairs, median after a warm-up)
from probe_score_views import scene, step_limit  # noqa: E402


def main(name, n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")

    with step_limit(240, f"scene {name} {n}^3"):
        kf, prm, nmap = scene(name, n)
    print(f"---- scene {name}, {n}^3, map of {nmap} frames, one MI355X")
    res = [n, n, n]
    pv, step = kf.volume_ptr("value")
    pw, _ = kf.volume_ptr("weight")
    good = True
    with step_limit(240, "grid and mask"):
        grid = torch.zeros(capi.view_grid_bytes(res), dtype=torch.uint8, device="cuda")
        capi.view_grid_build(pv, pw, step, res, grid)
        mask = torch.zeros(capi.frontier_mask_bytes(res), dtype=torch.uint8, device="cuda")
        ms = timed(torch, lambda: capi.frontier_mask(grid, res, mask), reps=20)
        out = torch.zeros(n ** 3, dtype=torch.uint8, device="cuda")
        capi.frontier_expand(mask, res, out)
        voxels = int(out.sum(dtype=torch.int64))
        del out
        print(f"mask {capi.frontier_mask_bytes(res) / 2**20:.0f} MiB, labels {capi.frontier_label_bytes(res) / 2**20:.0f} MiB")
        print(f"xs_frontier_mask: {ms * 1e3:9.1f} us (median of 20, one launch over {(n // 4) ** 3} bricks); frontier voxels {voxels}")
    labels = torch.zeros(n ** 3, dtype=torch.int32, device="cuda")
    capacity = 1 << 16
    ws = torch.zeros(capi.frontier_workspace_bytes(res, capacity), dtype=torch.uint8, device="cuda")
    rec = torch.zeros(capacity * 8, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    for cell in (0, 32, 64):
        with step_limit(300, f"labels at cell {cell}"):
            rounds = []
            ms = timed(torch, lambda: rounds.append(capi.frontier_label(mask, res, cell, labels, ws)), reps=5)
            a = labels.clone()
            capi.frontier_label(mask, res, cell, labels, ws)
            torch.cuda.synchronize()
            same = bool(torch.equal(a, labels))
            del a
            print(f"xs_frontier_label, cell {cell:2d}: {ms * 1e3:9.0f} us (median of 5, the whole call: seeding, {sorted(set(rounds))} rounds of {(n // 8) ** 3} "
                  f"workgroups in batches of 8 with a read-back each); two runs equal: {same}")
            good = good and same
        with step_limit(300, f"records at cell {cell}"):
            counts = []
            ms = timed(torch, lambda: counts.append(capi.frontier_clusters(mask, labels, res, capacity, rec, cnt, ws)), reps=5)
            a = rec.clone()
            count = capi.frontier_clusters(mask, labels, res, capacity, rec, cnt, ws)
            torch.cuda.synchronize()
            same = bool(torch.equal(a[:count * 8], rec[:count * 8])) and sorted(set(counts)) == [count]
            fits = count <= capacity
            total = int(rec[:count * 8].view(-1, 8)[:, 1].sum()) if fits else -1
            print(f"xs_frontier_clusters, cell {cell:2d}: {ms * 1e3:9.0f} us (median of 5, the whole call: compaction, the host's sort, accumulation); clusters {count}"
                  f"{'' if fits else ' (above the capacity of ' + str(capacity) + ': no records)'}; voxels in the records {total}; two runs equal: {same}")
            good = good and same and (not fits or total == voxels)
    kf.close()
    return good


if __name__ == "__main__":
    which = sys.argv[1:] or ["s1:512"]
    good = True
    for w in which:
        name, n = w.split(":")
        good = main(name, int(n)) and good
    if not good:
        print("DEFECT: two runs disagree, or the records do not account for every frontier voxel")
    sys.exit(0 if good else 1)
