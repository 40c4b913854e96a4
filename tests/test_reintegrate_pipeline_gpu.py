"""GPU: taking fused frames out and fusing them again at the orchestrator's level (KinectFusion.deintegrate, reintegrate, reintegrate_batch,
refine_frame) at 64^3 on the synthetic scene S1, six frames, with flag_use_gtPose and synth.s1_pose (seed included) as
the given poses, so that instances share poses bit for bit.  Volumes are compared with instances that never held the frame in question, within
the bound tests/reintegrate_cases.py derives, weights exactly; everything derived from the volume must follow the edited volume.

The refinement test tracks scene S3 normally.  Its distance to the true pose is d = |translation error| (m) + rotation angle (rad) x 1 m: with
the error it starts from, 1 cm and 0.5 degrees (0.0087 rad), both parts weigh about the same."""
import importlib
import threading

import numpy as np
import pytest

import merge_cases as mc
import reintegrate_cases as rc
from helpers import synth

pytestmark = pytest.mark.gpu
N, FRAMES, OUT = 64, 6, 3


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


def wrong(c2w):
    """c2w moved by 1 cm and turned by 0.5 degrees in the camera's own frame."""
    d = np.eye(4)
    d[:3, :3] = mc.rotation((0.3, 1.0, -0.2), np.radians(0.5))
    d[:3, 3] = np.array([0.6, -0.5, 0.62]) * 0.01 / np.linalg.norm([0.6, -0.5, 0.62])
    return c2w @ d


def given_poses(prm, ks, wrong_at=None):
    out = []
    for k in ks:
        c2w = synth.s1_transforms(k, prm)["c2w"]
        if k == wrong_at:
            c2w = wrong(c2w)
        out.append(synth.cmat(c2w.real, c2w.imag))
    return np.stack(out)


def fused(pl, prm, frames, ks, wrong_at=None):
    """(instance that fused frames ks at the given poses, the camera2volume each was fused at, bit for bit)."""
    kf = pl.KinectFusion(prm, gt_poses=given_poses(prm, ks, wrong_at))
    c2v = {}
    for k in ks:
        assert kf.process_frame(frames[k]) == 1
        c2v[k] = kf.camera2volume().copy()
    kf.synchronize()
    return kf, c2v


@pytest.fixture(scope="module")
def scene(dev):
    torch, capi, pl = dev
    prm = dict(synth.s1_params(N), flag_use_gtPose=True)
    frames = [torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda() for k in range(FRAMES)]
    ks = list(range(FRAMES))
    ref, c2v = fused(pl, prm, frames, ks)                                   # never modified by a test
    without, _ = fused(pl, prm, frames, [k for k in ks if k != OUT])        # nor this one
    # every frame's own observation (a fresh instance that fused it alone): the largest |Im t| per voxel, for the grad channel's bound
    Mg = np.zeros(N ** 3, np.float64)
    for k in ks:
        one, _ = fused(pl, prm, frames, [k])
        Mg = np.maximum(Mg, np.abs(one.volume()[2].astype(np.float64)))
        one.close()
    yield dict(prm=prm, frames=frames, ks=ks, ref=ref, c2v=c2v, without=without, Mg=Mg, ref_volume=tuple(x.copy() for x in ref.volume()),
               without_volume=tuple(x.copy() for x in without.volume()))
    ref.close()
    without.close()


def within(got, want, units, Mg, what):
    """Weights equal; values within units u, grads within units u x the voxel's largest |Im t|."""
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[1] > 0, want[1] > 0), what
    ev = np.abs(got[0].astype(np.float64) - want[0])
    eg = np.abs(got[2].astype(np.float64) - want[2])
    allow = rc.ALLOW * units * rc.U
    some = Mg > 0
    worst_g = float(np.max(eg[some] / Mg[some]) / rc.U) if some.any() else 0.0
    print(f"{what}: value error {ev.max() / rc.U:.2f} u, grad error {worst_g:.2f} u M, of {units} u allowed; grad error where M = 0: {eg[~some].max() if (~some).any() else 0.0}")
    assert ev.max() <= allow, (what, ev.max() / rc.U)
    assert (eg <= allow * Mg).all(), (what, worst_g)


def derived_state_follows(pl, kf, frames, prm):
    """The point cloud, the mesh over the rebuilt sign map and relocalize over the rebuilt band index are those of a fresh instance that
    received kf's volume bit for bit (merge_map under the identity into an empty volume is a copy and rebuilds everything)."""
    copy = pl.KinectFusion(prm)
    copy.merge_map(kf)
    a, b = kf.volume(), copy.volume()
    keep = a[1] > 0      # (the merge copies observed voxels)
    assert np.array_equal(a[1], b[1]) and mc.same_bits(a[0][keep], b[0][keep]) and mc.same_bits(a[2][keep], b[2][keep])
    pa, pc = kf.export_point_cloud(), copy.export_point_cloud()
    assert len(pa[0]) > 100 and mc.same_bits(pa[0], pc[0]) and np.array_equal(pa[1].view(np.uint32), pc[1].view(np.uint32))
    ma, mb = kf.export_mesh(), copy.export_mesh()
    assert len(ma.triangles) > 100 and mc.same_bits(ma.vertices, mb.vertices) and np.array_equal(ma.triangles, mb.triangles)
    start = kf.camera2volume().copy()
    start[0, 3, 0] += 0.01
    ra, rb = kf.relocalize(frames[FRAMES - 1], start), copy.relocalize(frames[FRAMES - 1], start)
    assert ra[0] and rb[0] and np.array_equal(ra[1].view(np.uint32), rb[1].view(np.uint32)) and np.array_equal(ra[2], rb[2])
    copy.close()


def test_deintegrate_equals_never_having_fused_the_frame(dev, scene):
    torch, capi, pl = dev
    prm, frames, ks = scene["prm"], scene["frames"], scene["ks"]
    a, c2v = fused(pl, prm, frames, ks)
    assert mc.same_bits(a.volume()[0], scene["ref_volume"][0]) and c2v[OUT].tobytes() == scene["c2v"][OUT].tobytes()
    gen, poses, frame_id, pose = a.volume_generation(), a.num_poses(), a.frame_id, a.camera2volume().copy()
    counts = a.deintegrate(frames[OUT], c2v[OUT])
    assert counts["removed"] > 1000 and counts["orphaned"] == 0 and counts["added"] == 0
    assert counts["removed"] == int((scene["ref_volume"][1] - scene["without_volume"][1]).sum())
    assert counts["emptied"] == int(((scene["ref_volume"][1] > 0) & (scene["without_volume"][1] == 0)).sum())
    # A: up to six additions and one removal; the other instance: up to five additions
    within(a.volume(), scene["without_volume"], rc.bound_u(FRAMES, 1) + rc.bound_u(FRAMES - 1, 0), scene["Mg"], "deintegrate")
    assert a.volume_generation() > gen and (a.num_poses(), a.frame_id) == (poses, frame_id) and np.array_equal(a.camera2volume(), pose)
    derived_state_follows(pl, a, frames, prm)
    a.close()


def test_reintegrate_at_the_same_pose(dev, scene):
    torch, capi, pl = dev
    prm, frames, ks = scene["prm"], scene["frames"], scene["ks"]
    a, c2v = fused(pl, prm, frames, ks)
    counts = a.reintegrate(frames[OUT], c2v[OUT], c2v[OUT])
    assert counts["removed"] == counts["added"] > 1000 and counts["orphaned"] == 0
    # six additions, a removal and an addition (3 * 5 -> 2 * 15 + 4 -> + 3) against six additions
    within(a.volume(), scene["ref_volume"], 2 * rc.bound_u(FRAMES, 0) + 4 + 3 + rc.bound_u(FRAMES, 0), scene["Mg"], "same pose")
    a.close()


def test_reintegrate_at_a_corrected_pose(dev, scene):
    torch, capi, pl = dev
    prm, frames, ks = scene["prm"], scene["frames"], scene["ks"]
    c, c2v_c = fused(pl, prm, frames, ks, wrong_at=OUT)
    right = scene["c2v"][OUT]
    assert not np.array_equal(c.volume()[1], scene["ref_volume"][1])          # the error is in the volume
    d = c2v_c[OUT][:3, 3, 0].astype(np.float64) - right[:3, 3, 0]
    assert 0.009 < np.linalg.norm(d) < 0.011
    poses, frame_id = c.num_poses(), c.frame_id
    record = c.world2camera().copy()
    counts = c.reintegrate(frames[OUT], c2v_c[OUT], right)
    assert counts["removed"] > 1000 and counts["added"] > 1000 and counts["orphaned"] == 0
    # the wrong frame's own |Im t| belongs to the voxel's observations as well
    one, _ = fused(pl, prm, frames, [OUT], wrong_at=OUT)
    Mg = np.maximum(scene["Mg"], np.abs(one.volume()[2].astype(np.float64)))
    one.close()
    within(c.volume(), scene["ref_volume"], 2 * rc.bound_u(FRAMES, 0) + 4 + 3 + rc.bound_u(FRAMES, 0), Mg, "corrected pose")
    assert (c.num_poses(), c.frame_id) == (poses, frame_id) and np.array_equal(c.world2camera(), record)     # no frame= given: the record stays
    derived_state_follows(pl, c, frames, prm)
    c.close()


def test_batch_equals_single_calls(dev, scene):
    torch, capi, pl = dev
    prm, frames, ks = scene["prm"], scene["frames"], scene["ks"]
    x, c2v = fused(pl, prm, frames, ks)
    y, _ = fused(pl, prm, frames, ks)
    which = [2, 4]
    news = [c2v[k].copy() for k in which]
    news[0][0, 3, 0] += 0.02
    news[1][1, 3, 0] -= 0.015
    cx = x.reintegrate_batch([frames[k] for k in which], [c2v[k] for k in which], news)
    cy = [y.reintegrate(frames[k], c2v[k], n) for k, n in zip(which, news)]
    assert cx == {k: cy[0][k] + cy[1][k] for k in cx} and cx["removed"] > 1000
    vx, vy = x.volume(), y.volume()
    assert mc.same_bits(vx[0], vy[0]) and np.array_equal(vx[1], vy[1]) and mc.same_bits(vx[2], vy[2])
    assert not mc.same_bits(vx[0], scene["ref_volume"][0])
    with pytest.raises(ValueError):
        x.reintegrate(frames[2], c2v[2], c2v[2], frame=x.num_poses())
    bad = c2v[2].copy()
    bad[1, 1, 0] = np.nan
    with pytest.raises(ValueError):
        x.deintegrate(frames[2], bad)
    after = x.volume()
    assert mc.same_bits(after[0], vx[0]) and np.array_equal(after[1], vx[1])
    x.close()
    y.close()


def pose_distance(c2v, truth):
    a = c2v[..., 0].astype(np.float64)
    dR = a[:3, :3].T @ truth[:3, :3]
    angle = np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))
    dt = np.linalg.norm(a[:3, 3] - truth[:3, 3])
    return dt + angle, dt, angle


def test_refine_frame_moves_towards_the_true_pose(dev):
    """Scene S3, tracked normally.  Frame 3 is moved to a pose off by 1 cm and 0.5 degrees (reintegrate), then refine_frame must end nearer to
    the true pose than it started, and return ok.  How much nearer, and how near relocalize gets on the map that still holds the frame, is
    printed (profiles/reintegrate_probe.txt records it), not asserted."""
    torch, capi, pl = dev
    prm = synth.s1_params(N)
    frames = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(FRAMES)]
    kf = pl.KinectFusion(prm)
    tracked = {}
    for k in range(FRAMES):
        assert kf.process_frame(frames[k]) == 1
        tracked[k] = kf.camera2volume().copy()
    w2v = np.eye(4)
    w2v[:3, 3] = [prm["init_x"], prm["init_y"], prm["init_z"]]
    truth = w2v @ synth.s1_pose(OUT)
    off = tracked[OUT].copy()
    moved = wrong(tracked[OUT][..., 0].astype(np.float64) + 1j * tracked[OUT][..., 1])
    off[..., 0], off[..., 1] = moved.real, moved.imag
    kf.reintegrate(frames[OUT], tracked[OUT], off)
    plain = kf.relocalize(frames[OUT], off)                 # the biased refinement: the map holds the frame at `off`
    poses, frame_id, others = kf.num_poses(), kf.frame_id, [kf.world2camera(k).copy() for k in range(FRAMES) if k != OUT]
    ok, refined, hist, counts = kf.refine_frame(frames[OUT], off, frame=OUT)      # (tracked normally, frame k's pose is record entry k)
    d0, d1, d2 = pose_distance(off, truth), pose_distance(refined, truth), pose_distance(plain[1], truth)
    print(f"refine_frame: start {d0}, refined {d1}, relocalize on the unmodified map {d2}, loss {hist[0]:.3e} -> {hist[-1]:.3e}")
    assert ok and counts["removed"] > 1000 and counts["added"] > 1000
    assert d1[0] < d0[0], (d0, d1)
    # frame= given: that entry of the record is the refined pose, the others, their number and the current pose stay
    w2c = kf.world2camera(OUT)
    back = w2v @ np.linalg.inv(w2c[..., 0].astype(np.complex128) + 1j * w2c[..., 1])
    assert np.allclose(back.real, refined[..., 0], atol=5e-6) and np.allclose(back.imag, refined[..., 1], atol=1e-9)
    assert (kf.num_poses(), kf.frame_id) == (poses, frame_id) == (FRAMES, FRAMES)
    assert all(np.array_equal(kf.world2camera(k), o) for k, o in zip([k for k in range(FRAMES) if k != OUT], others))
    assert np.array_equal(kf.camera2volume(), tracked[FRAMES - 1])
    kf.close()


def test_shard_mode_refuses(dev, scene):
    """Two ranks as threads on one GPU: the calls raise XsError (-2) on every rank and do nothing."""
    torch, capi, pl = dev
    sh = importlib.import_module("x-slam_amd.sharded")
    frames = scene["frames"]
    world = 2
    prm = dict(synth.s1_params(N), icp_shard_rows=False)
    lw = sh.LocalWorld(torch, world)
    shards = [sh.ShardedKinectFusion(prm, r, world, collective=lw.collective_for(r)) for r in range(world)]
    refused, errors, same = [0] * world, [], [False] * world

    def work(r):
        try:
            assert shards[r].process_frame(frames[0]) == 1
            before = tuple(x.copy() for x in shards[r].volume())
            c2v = shards[r].camera2volume()
            for call in (lambda: shards[r].deintegrate(frames[0], c2v), lambda: shards[r].reintegrate(frames[0], c2v, c2v),
                         lambda: shards[r].reintegrate_batch([frames[0]], [c2v], [c2v])):
                try:
                    call()
                except capi.XsError:
                    refused[r] += 1
            now = shards[r].volume()
            same[r] = mc.same_bits(now[0], before[0]) and np.array_equal(now[1], before[1])
            assert shards[r].process_frame(frames[1]) == 1
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            lw.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert refused == [3] * world and same == [True] * world
    for s in shards:
        s.close()
