"""Map differencing, measured on scene S1 at 512^3 after 30 tracked frames: the map against a device copy of itself
(the map merged into an empty 512^3 volume under the identity) under the identity, a shift by half a voxel along every axis and a rotation of
10 degrees about the volume's centre.  Per map: xs_tsdf_diff with the cull and with XS_DIFF_NO_CULL, and beside them the yardstick,
xs_tsdf_merge of the same source under the same transform into a second device copy of the map (restored outside the timed span before
every call): the three arms alternate inside one loop, three warm-up rounds, then the median of 20 calls each between hipEvent pairs (the
brick pre-pass included in all three).  Then, by a host clock around calls that end in a synchronise, the median of 5 after one warm-up: the
label and cluster passes over each of the two masks, and the whole orchestrator call (xs_kf_diff_volume, what diff_map runs: drain, diff,
two label and cluster passes, the records).  No time is a condition; the exit status is 1 only if the two arms of a diff disagree in a bit or
in a count.  One process; every GPU step runs under its own time limit (a watchdog that ends the process), and the first failure ends the
run.  Run in its own process:
    python profiles/tools/probe_diff.py > profiles/diff_probe.txt"""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_score_views import scene, step_limit  # noqa: E402


def main(n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")

    with step_limit(240, f"scene s1 {n}^3"):
        kf, prm, nmap = scene("s1", n)
    print(f"---- scene s1, {n}^3 against {n}^3, map of {nmap} frames, one MI355X")
    res = [n, n, n]
    vs = float(np.float32(prm["tsdf_voxel_size"]))
    max_weight = int(prm["max_integration_weight"])
    pv, step = kf.volume_ptr("value")
    pw, _ = kf.volume_ptr("weight")
    pg, _ = kf.volume_ptr("grad")
    with step_limit(120, "the copies"):
        other = [torch.zeros((n * n, n), dtype=t, device="cuda") for t in (torch.float32, torch.int32, torch.float32)]      # value, weight, grad
        ws = torch.zeros(capi.tsdf_merge_workspace_bytes(res, res), dtype=torch.uint8, device="cuda")
        capi.tsdf_merge(other[0], other[1], other[2], n * 4, res, pv, pw, pg, step, res, pl.merge_affine(np.eye(4), vs, vs), min_weight=1, max_weight=max_weight,
                        workspace=ws)
        torch.cuda.synchronize()
        dest = [t.clone() for t in other]                                                                                  # the merge's destination
    words = capi.frontier_mask_bytes(res) // 8
    masks = [[torch.full((words,), -1, dtype=torch.int64, device="cuda") for _ in range(2)] for _ in range(2)]          # [arm][class]
    counts = [torch.zeros(3, dtype=torch.int64, device="cuda") for _ in range(2)]
    written = torch.zeros(1, dtype=torch.int64, device="cuda")
    dws = torch.zeros(capi.tsdf_diff_workspace_bytes(res, res), dtype=torch.uint8, device="cuda")
    capacity = 1 << 18
    labels = torch.empty((n * n * n,), dtype=torch.int32, device="cuda")
    fws = torch.zeros(capi.frontier_workspace_bytes(res, capacity), dtype=torch.uint8, device="cuda")
    rec = torch.zeros((capacity * 8,), dtype=torch.int64, device="cuda")
    cnt = torch.zeros((1,), dtype=torch.int32, device="cuda")
    centre = 0.5 * n * vs * np.ones(3)
    a = np.radians(10.0)
    axis = np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    shift, rot = np.eye(4), np.eye(4)
    shift[:3, 3] = 0.5 * vs
    rot[:3, :3], rot[:3, 3] = R, centre - R @ centre
    good = True

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for name, T in (("identity", np.eye(4)), ("half-voxel shift", shift), ("rotation of 10 degrees", rot)):
        m = pl.merge_affine(T, vs, vs)
        arms = [("diff, cull", 0), ("diff, no cull", capi.DIFF_NO_CULL)]
        ms = {"diff, cull": [], "diff, no cull": [], "merge, cull": []}
        with step_limit(300, f"{name}: kernels"):
            for rep in range(23):                                       # three warm-up rounds, then 20 timed; the arms alternate
                for k, (arm, flags) in enumerate(arms):
                    counts[k].zero_()
                    t = timed(lambda: capi.tsdf_diff(pv, pw, step, res, other[0], other[1], n * 4, res, m, masks[k][0], masks[k][1], counts[k], min_weight=1,
                                                     lo=0.0, hi=0.5, flags=flags, workspace=dws))
                    if rep >= 3:
                        ms[arm].append(t)
                for d, o in zip(dest, other):
                    d.copy_(o)
                written.zero_()
                t = timed(lambda: capi.tsdf_merge(dest[0], dest[1], dest[2], n * 4, res, other[0], other[1], other[2], n * 4, res, m, min_weight=1,
                                                  max_weight=max_weight, written=written, workspace=ws))
                if rep >= 3:
                    ms["merge, cull"].append(t)
        c = [tuple(int(x) for x in t.cpu().numpy()) for t in counts]
        for arm, v in ms.items():
            extra = f"written {int(written.item())}" if arm.startswith("merge") else "compared {} only_this {} only_other {}".format(*c[0 if arm == "diff, cull" else 1])
            print(f"{name:24s} {arm:14s}: {np.median(v) * 1e3:9.1f} us (median of 20; min {min(v) * 1e3:.1f}); {extra}")
        same = c[0] == c[1] and all(torch.equal(masks[0][k], masks[1][k]) for k in range(2))
        print(f"{name:24s} the two diff arms equal: {same}; diff with the cull / merge with the cull = {np.median(ms['diff, cull']) / np.median(ms['merge, cull']):.2f}")
        good = good and same
        with step_limit(300, f"{name}: label and clusters"):
            for k, cls in enumerate(("only_this", "only_other")):
                ts, found, rounds = [], 0, 0
                for rep in range(6):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    rounds = capi.frontier_label(masks[0][k], res, 0, labels, fws)
                    t1 = time.perf_counter()
                    found = capi.frontier_clusters(masks[0][k], labels, res, capacity, rec, cnt, fws)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if rep >= 1:
                        ts.append((t1 - t0, t2 - t1))
                lab, clu = np.median([t[0] for t in ts]) * 1e3, np.median([t[1] for t in ts]) * 1e3
                print(f"{name:24s} {cls:10s}: label {lab:8.2f} ms ({rounds} rounds), clusters {clu:8.2f} ms ({found} clusters; capacity {capacity}); host clock, median of 5")
        with step_limit(300, f"{name}: the orchestrator's call"):
            u64p = C.POINTER(C.c_uint64)
            recs = [np.zeros((capacity, 8), np.uint64) for _ in range(2)]
            nt, no, c3 = C.c_int(0), C.c_int(0), np.zeros(3, np.uint64)
            r3, t16 = np.array(res, np.int32), np.ascontiguousarray(T, np.float64)
            ts = []
            for rep in range(6):
                t0 = time.perf_counter()
                rc = pl._lib.xs_kf_diff_volume(kf.h, other[0].data_ptr(), other[1].data_ptr(), n * 4, r3.ctypes.data_as(pl._i32p), vs, kf.tranc_dist(),
                                               t16.ctypes.data_as(pl._f64p), 1, 0.0, 0.5, 0, 8, capacity, recs[0].ctypes.data_as(u64p), C.byref(nt),
                                               recs[1].ctypes.data_as(u64p), C.byref(no), c3.ctypes.data_as(C.POINTER(C.c_ulonglong)), None, None)
                ts.append(time.perf_counter() - t0)
                assert rc in (1, -4), rc
            print(f"{name:24s} xs_kf_diff_volume (diff_map; min_size 8, no dense masks): {np.median(ts[1:]) * 1e3:8.2f} ms (host clock, median of 5; rc {rc}); "
                  f"clusters kept {nt.value} + {no.value}; counts {tuple(int(x) for x in c3)}")
    kf.close()
    return good


if __name__ == "__main__":
    ok = main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
    if not ok:
        print("DEFECT: the cull changed the result")
    sys.exit(0 if ok else 1)
