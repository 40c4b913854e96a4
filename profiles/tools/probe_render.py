"""Rendering views of the map, measured on scene S1 at 512^3 after 30 tracked frames, 640 x 480 images at the tracked
pose (and, for P > 1, at poses turned away from it in steps).  Alternating in one loop, three warm-up rounds, then the median of 20 calls each
between hipEvent pairs (pose upload, zeroing of the counts and, with the cull, the read-back of the mask's header included):
  - xs_render_views with the cull at P = 1, 8 and 64, every output wanted;
  - P = 1 without the cull;
  - xs_render_mask_build alone;
  - as the yardstick xs_raycast_ex at the same pose: its exact path and its sign-map path (vertex and normal maps in complex arithmetic, one
    view per launch).
The mask lookup of the march exists in one variant, reads through L2 with the word kept in a register; a per-workgroup copy in LDS was not built,
so that arm is absent.  No time is a condition; the exit status is 1 only if the culled launch and the launch without the cull disagree in a
bit.  One process; every GPU step runs under its own time limit, and the first failure ends the run.  Run in its own process:
    python profiles/tools/probe_render.py > profiles/render_probe.txt"""
import importlib
import os
import sys

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
    from helpers import intr_of, tranc_dist
    import merge_cases as mc
    nmap = 30
    prm = synth.s1_params(n, seed=None)
    with step_limit(300, f"scene s1 {n}^3"):
        kf = pl.KinectFusion(prm)
        for k in range(nmap):
            assert kf.process_frame(torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda()) == 1
        kf.synchronize()
    print(f"---- scene s1, {n}^3, map of {nmap} tracked frames, one MI355X, images of 640 x 480")
    W, H = synth.WIDTH, synth.HEIGHT
    res, vs, k4 = [n, n, n], float(np.float32(prm["tsdf_voxel_size"])), intr_of(prm)
    (pv, step), (pw, _), (pg, _) = kf.volume_ptr("value"), kf.volume_ptr("weight"), kf.volume_ptr("grad")
    c2v = kf.camera2volume()[..., 0].astype(np.float64)
    R, t = [], []
    for p in range(64):                      # view p: the tracked pose turned by p / 4 degrees about the camera's y
        m = c2v.copy()
        m[:3, :3] = c2v[:3, :3] @ mc.rotation((0.0, 1.0, 0.0), np.radians(p / 4))
        R.append(m[:3, :3])
        t.append(m[:3, 3])
    R, t = np.array(R, np.float32), np.array(t, np.float32)
    with step_limit(120, "buffers"):
        ws = torch.zeros(capi.render_workspace_bytes(res), dtype=torch.uint8, device="cuda")
        depth = torch.empty((64, H, W), dtype=torch.float32, device="cuda")
        depth16 = torch.empty((64, H, W), dtype=torch.int16, device="cuda")
        normal = torch.empty((64, 3, H, W), dtype=torch.float32, device="cuda")
        shade = torch.empty((64, H, W), dtype=torch.uint8, device="cuda")
        counts = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
        vm = torch.zeros((3 * H, W, 2), dtype=torch.float32, device="cuda")
        nm = torch.zeros((3 * H, W, 2), dtype=torch.float32, device="cuda")
        rws = torch.zeros(H * W, dtype=torch.float32, device="cuda")
        shift = capi.raycast_signmap_shift(k4, vs, tranc_dist(prm))
        smap = torch.zeros(capi.signmap_bytes(res, shift), dtype=torch.uint8, device="cuda") if shift else None
        if shift:
            capi.signmap_rebuild(smap, res, shift, tranc_dist(prm), pv, step)
        capi.render_mask_build(pv, pw, step, res, ws)
        torch.cuda.synchronize()
    eye, zero = synth.cmat(np.eye(3)), synth.cmat(np.zeros(3))

    def render(P, cull):
        capi.render_views(R[:P], t[:P], k4, H, W, pv, pw, step, res, vs, ws, opts=capi.render_opts(cull=cull), depth=depth, depth_u16=depth16, normal=normal,
                          shade=shade, counts=counts)

    def raycast(**kw):
        capi.raycast(k4, synth.cmat(R[0]), synth.cmat(t[0]), eye, zero, tranc_dist(prm), res, vs, pv, pg, step, vm, nm, W * 8, H, W, workspace=rws, **kw)

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    arms = {"render P = 1, cull": (1, lambda: render(1, True)), "render P = 8, cull": (8, lambda: render(8, True)), "render P = 64, cull": (64, lambda: render(64, True)),
            "render P = 1, no cull": (1, lambda: render(1, False)), "mask build": (0, lambda: capi.render_mask_build(pv, pw, step, res, ws)),
            "raycast_ex, exact path": (1, lambda: raycast())}
    if shift:
        arms["raycast_ex, sign-map path"] = (1, lambda: raycast(signmap=smap, signmap_shift=shift, signmap_tranc_dist=tranc_dist(prm)))
    ms = {a: [] for a in arms}
    with step_limit(600, "kernels"):
        for rep in range(23):
            for arm, (P, call) in arms.items():
                d = timed(call)
                if rep >= 3:
                    ms[arm].append(d)
        for arm, (P, call) in arms.items():
            med = float(np.median(ms[arm]))
            rays = f"; {med * 1e3 / P:8.1f} us per view, {P * H * W / (med * 1e-3) / 1e6:7.1f} Mrays/s" if P else ""
            print(f"{arm:26s}: {med * 1e3:9.1f} us (median of 20; min {min(ms[arm]) * 1e3:.1f}){rays}")
    with step_limit(120, "cull against no cull"):
        outs = []
        for cull in (True, False):
            render(1, cull)
            torch.cuda.synchronize()
            outs.append([x[:1].clone() for x in (depth, depth16, normal, shade, counts)])
        same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(*outs))
        c = outs[0][4][0].cpu().numpy().view(np.uint32)
        print(f"view 0: hit, backface, rejected, none = {c.tolist()} of {H * W} rays; the launch without the cull gives the same bytes: {same}")
    kf.close()
    return same


if __name__ == "__main__":
    good = main(int(sys.argv[1]) if len(sys.argv) > 1 else 512)
    if not good:
        print("DEFECT: the cull changed the result")
    sys.exit(0 if good else 1)
