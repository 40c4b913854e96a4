"""Volume merge, measured on scene S1 at 512^3 after 30 tracked frames: the map merged into an empty 512^3 volume
under the identity, a shift by half a voxel along every axis and a rotation of 10 degrees about the volume's centre, each with the cull and
with XS_MERGE_NO_CULL.  Per arm: the median of 20 xs_tsdf_merge calls (the brick pre-pass included) between hipEvent pairs after a warm-up,
the destination cleared outside the timed span before every call; beside it the algorithmic bytes — 12 read and 12 written per written
voxel, plus 12 per source voxel under the destination's image — and what they come to per second.  No time is a condition; the exit status
is 1 only if the two arms of a map disagree in a bit or in the count.  One process; every GPU step runs under its own time limit (a watchdog
that ends the process), and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_merge.py > profiles/merge_probe.txt"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from probe_score_views import scene, step_limit  # noqa: E402


def image_voxels(torch, m12, res, sres):
    """Source voxels whose centre lies under the destination volume: the inverse of the affine map takes them into [-0.5, res - 0.5)."""
    A = np.asarray(m12[:9], np.float64).reshape(3, 3)
    Ai = torch.from_numpy(np.linalg.inv(A)).cuda()
    o = torch.from_numpy(np.asarray(m12[9:], np.float64)).cuda()
    hi = torch.tensor([r - 0.5 for r in res], dtype=torch.float64, device="cuda")
    x = torch.arange(sres[0], dtype=torch.float64, device="cuda")[None, None, :]
    y = torch.arange(sres[1], dtype=torch.float64, device="cuda")[None, :, None]
    total = 0
    for z0 in range(0, sres[2], 16):
        z = torch.arange(z0, min(z0 + 16, sres[2]), dtype=torch.float64, device="cuda")[:, None, None]
        s = [x - o[0], y - o[1], z - o[2]]
        ok = None
        for a in range(3):
            d = Ai[a, 0] * s[0] + Ai[a, 1] * s[1] + Ai[a, 2] * s[2]
            t = (d >= -0.5) & (d < hi[a])
            ok = t if ok is None else ok & t
        total += int(ok.sum())
    return total


def main(n):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")

    with step_limit(240, f"scene s1 {n}^3"):
        kf, prm, nmap = scene("s1", n)
    print(f"---- scene s1, {n}^3 into {n}^3, map of {nmap} frames, one MI355X")
    res = [n, n, n]
    vs = float(np.float32(prm["tsdf_voxel_size"]))
    pv, step = kf.volume_ptr("value")
    pw, _ = kf.volume_ptr("weight")
    pg, _ = kf.volume_ptr("grad")
    dv = torch.zeros((n * n, n), dtype=torch.float32, device="cuda")
    dw = torch.zeros((n * n, n), dtype=torch.int32, device="cuda")
    dg = torch.zeros((n * n, n), dtype=torch.float32, device="cuda")
    ws = torch.zeros(capi.tsdf_merge_workspace_bytes(res, res), dtype=torch.uint8, device="cuda")
    written = torch.zeros(1, dtype=torch.int64, device="cuda")
    centre = 0.5 * n * vs * np.ones(3)
    a = np.radians(10.0)
    axis = np.array([0.3, 1.0, 0.2]) / np.linalg.norm([0.3, 1.0, 0.2])
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    R = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    shift, rot = np.eye(4), np.eye(4)
    shift[:3, 3] = 0.5 * vs
    rot[:3, :3], rot[:3, 3] = R, centre - R @ centre
    good = True
    for name, T in (("identity", np.eye(4)), ("half-voxel shift", shift), ("rotation of 10 degrees", rot)):
        m = pl.merge_affine(T, vs, vs)
        with step_limit(120, f"image of {name}"):
            under = image_voxels(torch, m, res, res)
        results = []
        for flags, arm in ((0, "cull"), (capi.MERGE_NO_CULL, "no cull")):
            with step_limit(300, f"{name}, {arm}"):
                ms = []
                for rep in range(23):                                   # three warm-up calls, then 20 timed
                    dv.zero_(); dw.zero_(); dg.zero_(); written.zero_()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    capi.tsdf_merge(dv, dw, dg, n * 4, res, pv, pw, pg, step, res, m, min_weight=1, max_weight=int(prm["max_integration_weight"]), flags=flags,
                                    written=written, workspace=ws)
                    e1.record()
                    e1.synchronize()
                    if rep >= 3:
                        ms.append(e0.elapsed_time(e1))
                wr = int(written.item())
                bytes_ = 24 * wr + 12 * under
                med = float(np.median(ms))
                print(f"{name:24s} {arm:8s}: {med * 1e3:9.1f} us (median of 20; min {min(ms) * 1e3:.1f}); written {wr}; source voxels under the image {under}; "
                      f"algorithmic bytes {bytes_ / 2**20:.0f} MiB = {bytes_ / med / 1e9:.2f} TB/s")
                results.append((wr, dv.clone(), dw.clone(), dg.clone()))
        same = results[0][0] == results[1][0] and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(results[0][1:], results[1][1:]))
        print(f"{name:24s} the two arms equal: {same}")
        good = good and same
        del results
    kf.close()
    return good


if __name__ == "__main__":
    ok = main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
    if not ok:
        print("DEFECT: the cull changed the result")
    sys.exit(0 if ok else 1)
