"""The brick-sparse checkpoint, measured on scene S1 at 512^3 after 30 tracked frames.  The kernels between hipEvent
pairs, three warm-up rounds and the median of 20 calls each: xs_tsdf_pack_classify (the classify kernel and the three launches of the scan; its
read rate is 12 bytes per voxel over the time, given as a fraction of 8 TB/s), xs_tsdf_pack_gather and xs_tsdf_unpack of the whole volume in one
range (the unpack into a second set of arrays, compared with the map afterwards).  Then, by a host clock around calls that end in a synchronise,
dense against sparse in the same run, the median of 3 after one warm-up: save_checkpoint, load_checkpoint into a second instance, and
merge_checkpoint into a third under the identity; and the two file sizes.  The files go to a temporary directory that is removed.  No time is a
condition; the exit status is 1 only if the unpacked volume, or a volume loaded from the sparse file, differs from the map in a bit.  One process;
every GPU step runs under its own time limit (a watchdog that ends the process), and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_pack.py > profiles/pack_probe.txt"""
import importlib
import os
import sys
import tempfile
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
    print(f"---- scene s1, {n}^3, map of {nmap} frames, one MI355X")
    res = [n, n, n]
    pv, step = kf.volume_ptr("value")
    pw, _ = kf.volume_ptr("weight")
    pg, _ = kf.volume_ptr("grad")
    nb = capi.tsdf_pack_bricks(res)
    cls = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    offsets = torch.zeros(nb + 1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(capi.tsdf_pack_workspace_bytes(res), dtype=torch.uint8, device="cuda")

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def median_of_20(call):
        ts = [timed(call) for _ in range(23)][3:]
        return float(np.median(ts)), float(min(ts))

    with step_limit(120, "classify"):
        med, lo = median_of_20(lambda: capi.tsdf_pack_classify(pv, pw, pg, step, res, cls, offsets, ws))
        words = int(offsets[-1].item())
        hist = np.bincount(cls.cpu().numpy(), minlength=8).tolist()
    rate = 12.0 * n ** 3 / (med * 1e-3)
    print(f"classify + offsets : {med * 1e3:9.1f} us (median of 20; min {lo * 1e3:.1f}); {rate / 1e12:.2f} TB/s read = {rate / 8e12:.2f} of 8 TB/s")
    print(f"bricks {nb}, per class {hist}; payload {words} words = {4 * words / (12 * n ** 3):.4f} of the dense 12 bytes per voxel")
    payload = torch.zeros(words, dtype=torch.int32, device="cuda")
    with step_limit(120, "gather"):
        med, lo = median_of_20(lambda: capi.tsdf_pack_gather(pv, pw, pg, step, res, cls, offsets, 0, nb, payload))
    print(f"gather, one range  : {med * 1e3:9.1f} us (median of 20; min {lo * 1e3:.1f})")
    with step_limit(120, "unpack"):
        out = [torch.full((n * n, n), -1, dtype=torch.int32, device="cuda") for _ in range(3)]
        med, lo = median_of_20(lambda: capi.tsdf_unpack(out[0], out[1], out[2], n * 4, res, cls, offsets, 0, nb, payload))
        good = all(np.array_equal(o.cpu().numpy().reshape(-1).view(np.uint32), np.ascontiguousarray(h).view(np.uint32)) for o, h in zip(out, kf.volume()))
        print(f"unpack, one range  : {med * 1e3:9.1f} us (median of 20; min {lo * 1e3:.1f}); the unpacked volume equals the map: {good}")
    del out, payload

    def wall(call, reps=4):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts[1:])) * 1e3

    with tempfile.TemporaryDirectory() as d:
        paths = {"dense": os.path.join(d, "dense.ckpt"), "sparse": os.path.join(d, "sparse.ckpt")}
        with step_limit(600, "save"):
            t_save = {"dense": wall(lambda: kf.save_checkpoint(paths["dense"])), "sparse": wall(lambda: kf.save_checkpoint(paths["sparse"], sparse=True))}
        size = {k: os.path.getsize(p) for k, p in paths.items()}
        print(f"file bytes         : dense {size['dense']}, sparse {size['sparse']} ({size['sparse'] / size['dense']:.4f})")
        map_volume = kf.volume()
        b, c = pl.KinectFusion(prm), pl.KinectFusion(prm)
        t_load, t_merge = {}, {}
        with step_limit(600, "load"):
            for k in ("dense", "sparse"):
                t_load[k] = wall(lambda: b.load_checkpoint(paths[k]))
                same = all(np.array_equal(np.ascontiguousarray(x).view(np.uint32), np.ascontiguousarray(y).view(np.uint32)) for x, y in zip(b.volume(), map_volume))
                good = good and same
                print(f"load_checkpoint    : {k:6s} {t_load[k]:9.1f} ms (host clock, median of 3); the loaded volume equals the map: {same}")
        with step_limit(600, "merge"):
            for k in ("dense", "sparse"):
                t_merge[k] = wall(lambda: c.merge_checkpoint(paths[k]))
        for k in ("dense", "sparse"):
            print(f"{k:6s}: save_checkpoint {t_save[k]:9.1f} ms, load_checkpoint {t_load[k]:9.1f} ms, merge_checkpoint {t_merge[k]:9.1f} ms (host clock, median of 3)")
        print(f"dense / sparse     : save {t_save['dense'] / t_save['sparse']:.1f}, load {t_load['dense'] / t_load['sparse']:.1f}, "
              f"merge_checkpoint {t_merge['dense'] / t_merge['sparse']:.1f}")
        b.close()
        c.close()
    kf.close()
    return good


if __name__ == "__main__":
    ok = main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
    if not ok:
        print("DEFECT: a volume came back from the sparse format with other bits")
    sys.exit(0 if ok else 1)
