"""Time of one mesh export (xs_extract_mesh, count + fill, two stream synchronisations) on scene S1 after 30 frames, at 256^3, 512^3 and
1024^3, with and without a sign map (rebuilt from the volume, brick shift 3), and the fraction of 8 TB/s it reaches on the algorithmic
bytes: 8 B per voxel of value + weight over the bricks read, 8 B of grad per vertex, and the outputs.  Run in its own process:
    python profiles/tools/probe_mesh.py [n ...] > profiles/mesh_probe.txt"""
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(sizes):
    import torch
    capi = importlib.import_module("x-slam_amd.capi")
    pl = importlib.import_module("x-slam_amd.pipeline")
    synth = importlib.import_module("x-slam_amd.synth")
    print("n     signmap  ms/export (median of 7)  V          T          bricks_read  GB_algorithmic  fraction_of_8TB/s")
    for n in sizes:
        prm = synth.s1_params(n)
        kf = pl.KinectFusion(prm)
        for k in range(30):
            assert kf.process_frame(torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda()) == 1
        kf.synchronize()
        res = [n, n, n]
        value, step = kf.volume_ptr("value")
        weight, _ = kf.volume_ptr("weight")
        grad, _ = kf.volume_ptr("grad")
        shift = 3
        sm = torch.zeros(capi.signmap_bytes(res, shift), dtype=torch.uint8, device="cuda")
        capi.signmap_rebuild(sm, res, shift, kf.tranc_dist(), value, step)
        torch.cuda.synchronize()
        nb = (n >> shift) ** 3
        dil = sm[64 + 320 * 4 + ((nb + 255) & ~255):][:nb]
        bricks_read = int((dil != 0).sum())
        for use_map in (False, True):
            opts = capi.mesh_opts(res=res, want_normals=True, signmap=sm if use_map else None, signmap_shift=shift)
            ws = torch.empty(capi.mesh_workspace_bytes(res, opts), dtype=torch.uint8, device="cuda")
            _, V, T = capi.extract_mesh_raw(value, weight, grad, step, res, prm["tsdf_voxel_size"], opts, None, None, None, None, 0, None, 0, ws)
            f = lambda: torch.empty((V, 3), dtype=torch.float32, device="cuda")
            out = (f(), f(), f(), torch.empty(V, dtype=torch.int64, device="cuda"), torch.empty((T, 3), dtype=torch.int32, device="cuda"))
            ts = []
            for _ in range(7):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc, _, _ = capi.extract_mesh_raw(value, weight, grad, step, res, prm["tsdf_voxel_size"], opts, out[0], out[1], out[2], out[3], V,
                                                 out[4], T, ws)
                ts.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
            ms = float(np.median(ts))
            voxels = bricks_read * (1 << 3 * shift) if use_map else n ** 3
            gb = (8.0 * voxels + 8.0 * V + V * (12 + 12 + 12 + 8) + T * 12) / 1e9
            print(f"{n:<5d} {'on' if use_map else 'off':<8s} {ms:<24.3f} {V:<10d} {T:<10d} {bricks_read if use_map else nb:<12d} {gb:<15.3f} "
                  f"{gb / (ms * 1e-3) / 8000.0:.3f}", flush=True)
        del kf, sm, ws, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [256, 512, 1024])
