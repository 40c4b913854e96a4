"""GPU: rendering views at the orchestrator's level (KinectFusion.render_views, render_map, render_checkpoint) at 64^3 on
the synthetic scene S1, six frames at given poses, as tests/test_reintegrate_pipeline_gpu.py.  Every image is compared for equal bits with
the float32 model of tests/render_cases.py run on the downloaded volume."""
import importlib
import threading

import numpy as np
import pytest

import merge_cases as mc
import render_cases as rc
from helpers import synth

pytestmark = pytest.mark.gpu
N, FRAMES = 64, 6
SIZE = (120, 160)            # the images the model is run on: a quarter of the camera's, with its intrinsics scaled to match


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


def given_poses(prm, ks):
    out = []
    for k in ks:
        c2w = synth.s1_transforms(k, prm)["c2w"]
        out.append(synth.cmat(c2w.real, c2w.imag))
    return np.stack(out)


def cube(vol):
    return vol[0].reshape(N, N, N), vol[1].reshape(N, N, N)


def moved(c2v, t_cm, angle_deg, axis=(0.3, 1.0, -0.2)):
    """c2v [4, 4, 2] moved by t_cm and turned by angle_deg in the camera's own frame."""
    d = np.eye(4)
    d[:3, :3] = mc.rotation(axis, np.radians(angle_deg))
    d[:3, 3] = np.array([0.6, -0.5, 0.62]) * 0.01 * t_cm / np.linalg.norm([0.6, -0.5, 0.62])
    out = c2v.copy()
    m = (c2v[..., 0].astype(np.float64) + 1j * c2v[..., 1]) @ d
    out[..., 0], out[..., 1] = m.real, m.imag
    return out


def small_intr(prm):
    return np.array([prm["fx"] / 4, prm["fy"] / 4, (prm["cx"] + 0.5) / 4 - 0.5, (prm["cy"] + 0.5) / 4 - 0.5], np.float32)


def model(kf, prm, poses, **kw):
    value, weight = cube(kf.volume())
    m = np.ascontiguousarray(poses, np.float32).reshape(-1, 4, 4, 2)[..., 0]
    opts = dict(t_near=0.2, t_far=5.0, step=0.0, min_weight=1)
    opts.update(kw)
    return rc.render((value, weight), np.float32(prm["tsdf_voxel_size"]), m[:, :3, :3], m[:, :3, 3], small_intr(prm), SIZE[0], SIZE[1], **opts)


ALL = ("depth", "depth_u16", "normal", "shade", "counts")


def assert_same(got, want, what=""):
    for k in ALL:
        assert rc.same_output(k, getattr(got, k), want[k] if isinstance(want, dict) else getattr(want, k)), (what, k)


@pytest.fixture(scope="module")
def scene(dev):
    torch, capi, pl = dev
    prm = dict(synth.s1_params(N), flag_use_gtPose=True)
    frames = [torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda() for k in range(FRAMES)]
    a = pl.KinectFusion(prm, gt_poses=given_poses(prm, range(FRAMES)))      # never modified by a test
    c2v = {}
    for k in range(FRAMES):
        assert a.process_frame(frames[k]) == 1
        c2v[k] = a.camera2volume().copy()
    a.synchronize()
    poses = np.stack([a.camera2volume(), moved(a.camera2volume(), 30.0, 12.0), moved(c2v[0], -20.0, -8.0, axis=(1.0, 0.2, 0.1))])
    yield dict(a=a, prm=prm, frames=frames, c2v=c2v, poses=poses)
    a.close()


def test_render_views_equals_the_model(dev, scene):
    torch, capi, pl = dev
    a, prm, poses = scene["a"], scene["prm"], scene["poses"]
    gen = a.volume_generation()
    want = model(a, prm, poses)
    print("hit, backface, rejected, none per view:", want["counts"].tolist())
    assert (want["counts"][:, 0] > SIZE[0] * SIZE[1] // 10).all()                   # every view shows the surface
    for cull in (True, False, True):
        got = a.render_views(poses, intr=small_intr(prm), size=SIZE, outputs=ALL, cull=cull)
        assert isinstance(got, pl.RenderedViews)
        assert_same(got, want, cull)
    # real poses [P, 4, 4] are the complex ones' real parts; one pose alone is the first of three; an output not asked for is None
    real = a.render_views(poses[..., 0], intr=small_intr(prm), size=SIZE, outputs=ALL)
    assert_same(real, want)
    one = a.render_views(poses[0], intr=small_intr(prm), size=SIZE, outputs=("depth", "counts"))
    assert one.normal is None and one.shade is None and one.depth_u16 is None
    assert rc.same_output("depth", one.depth, want["depth"][:1]) and np.array_equal(one.counts, want["counts"][:1])
    # the other options reach the kernel
    kw = dict(t_near=0.5, t_far=4.0, step=0.07, min_weight=2)
    got = a.render_views(poses, intr=small_intr(prm), size=SIZE, outputs=ALL, **kw)
    assert_same(got, model(a, prm, poses, **kw), kw)
    # the defaults: the configuration's camera; 70 views take two launches
    full = a.render_views(poses[:1])
    assert full.depth.shape == (1, synth.HEIGHT, synth.WIDTH) and full.normal.shape == (1, 3, synth.HEIGHT, synth.WIDTH) and full.shade.dtype == np.uint8
    assert full.depth_u16 is None and full.counts is None and (full.depth > 0).mean() > 0.1
    many = a.render_views(np.concatenate([poses] * 23 + [poses[:1]]), intr=small_intr(prm), size=SIZE, outputs=("depth", "counts"))
    assert many.depth.shape[0] == 70 and rc.same_output("depth", many.depth[66:69], want["depth"]) and np.array_equal(many.counts[69], want["counts"][0])
    assert a.volume_generation() == gen
    for call in (lambda: a.render_views(poses, size=(0, 5)), lambda: a.render_views(poses, size=(4097, 5)), lambda: a.render_views(poses, t_near=1.0, t_far=1.0),
                 lambda: a.render_views(poses, step=-1.0), lambda: a.render_views(poses, step=1e-4), lambda: a.render_views(poses, outputs=()),
                 lambda: a.render_views(poses, outputs=("colour",)), lambda: a.render_views(np.zeros((2, 3, 3))),
                 lambda: a.render_views(poses, intr=(0.0, 100.0, 1.0, 1.0)), lambda: a.render_views(np.full((1, 4, 4), np.nan))):
        with pytest.raises(ValueError):
            call()


def test_checkpoints_and_another_instance_render_the_same(dev, scene, tmp_path):
    torch, capi, pl = dev
    a, prm, poses = scene["a"], scene["prm"], scene["poses"]
    kw = dict(intr=small_intr(prm), size=SIZE, outputs=ALL)
    want = a.render_views(poses, **kw)
    dense, sparse = str(tmp_path / "a.ckpt"), str(tmp_path / "a.sparse")
    a.save_checkpoint(dense)
    a.save_checkpoint(sparse, sparse=True)
    b = pl.KinectFusion(prm)
    for cull in (True, False):
        assert_same(b.render_checkpoint(dense, poses, cull=cull, **kw), want, "dense")
        assert_same(b.render_checkpoint(sparse, poses, cull=cull, **kw), want, "sparse")
        assert_same(b.render_map(a, poses, cull=cull, **kw), want, "map")
    assert_same(a.render_checkpoint(dense, poses, **kw), want, "its own checkpoint")
    assert not b.render_views(poses, **kw).depth.any()                              # b's own map is empty, and stays so
    for call in (lambda: b.render_checkpoint(str(tmp_path / "missing"), poses), lambda: b.render_map(b, poses), lambda: b.render_map(a, poses, size=(0, 7))):
        with pytest.raises(ValueError):
            call()
    b.close()


def test_the_cached_mask_follows_the_edited_volume(dev, scene):
    """A fresh instance renders nothing and caches an empty mask; after merge_map, and again after reintegrate, the render is the model's on
    the new volume (a stale mask would hide the surface)."""
    torch, capi, pl = dev
    a, prm, poses, frames, c2v = scene["a"], scene["prm"], scene["poses"], scene["frames"], scene["c2v"]
    kw = dict(intr=small_intr(prm), size=SIZE, outputs=ALL)
    c = pl.KinectFusion(prm)
    empty = c.render_views(poses, **kw)
    assert not empty.depth.any() and (empty.counts[:, 3] == SIZE[0] * SIZE[1]).all()
    c.merge_map(a)
    after_merge = c.render_views(poses, **kw)
    assert_same(after_merge, model(c, prm, poses), "after merge_map")
    assert_same(after_merge, a.render_views(poses, **kw), "the merged copy renders as the original")
    c.close()
    # an instance that fused the frames itself, rendered once (its mask is cached), then edited: frame 3 moved by 4 cm and 2 degrees
    e = pl.KinectFusion(prm, gt_poses=given_poses(prm, range(FRAMES)))
    for k in range(FRAMES):
        assert e.process_frame(frames[k]) == 1
    before_edit = e.render_views(poses, **kw)
    assert_same(before_edit, model(e, prm, poses), "before the edit")
    e.reintegrate(frames[3], c2v[3], moved(c2v[3], 4.0, 2.0))
    after_edit = e.render_views(poses, **kw)
    assert_same(after_edit, model(e, prm, poses), "after reintegrate")
    assert not rc.same_output("depth", after_edit.depth, before_edit.depth)
    assert_same(e.render_views(poses, cull=False, **kw), after_edit, "cull off")
    e.close()


def pose_distance(c2v, other):
    x, y = c2v[..., 0].astype(np.float64), other[..., 0].astype(np.float64)
    dR = x[:3, :3].T @ y[:3, :3]
    angle = np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))
    dt = np.linalg.norm(x[:3, 3] - y[:3, 3])
    return dt + angle, dt, angle


def test_a_rendered_depth_stands_in_for_a_frame(dev):
    """Scene S3, tracked normally.  The depth_u16 rendered at the tracked pose, left on the device, goes to relocalize from a start 1 cm and 0.5
    degrees off: it must end nearer the render pose than it started (a condition on direction; the distances are printed, DESIGN.md section
    4.28 quotes them)."""
    torch, capi, pl = dev
    prm = synth.s1_params(N)
    kf = pl.KinectFusion(prm)
    for k in range(FRAMES):
        assert kf.process_frame(torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda()) == 1
    pose = kf.camera2volume().copy()
    views = kf.render_views(pose, outputs=("depth_u16", "depth", "counts"), device=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (views.depth_u16, views.depth, views.counts)) and views.normal is None
    assert views.depth_u16.shape == (1, synth.HEIGHT, synth.WIDTH) and views.depth_u16.element_size() == 2
    host = kf.render_views(pose, outputs=("depth_u16", "depth", "counts"))
    assert np.array_equal(views.depth_u16.cpu().numpy().view(np.uint16), host.depth_u16) and rc.same_output("depth", views.depth.cpu().numpy(), host.depth)
    assert np.array_equal(views.counts.cpu().numpy().view(np.uint32), host.counts)
    mm = host.depth_u16[0]
    assert np.array_equal(mm[mm > 0], np.rint(host.depth[0][mm > 0] * np.float32(1000.0)).astype(np.uint16)) and (mm > 0).mean() > 0.2
    start = moved(pose, 1.0, 0.5)
    ok, refined, hist = kf.relocalize(views.depth_u16[0], start)
    d0, d1 = pose_distance(start, pose), pose_distance(refined, pose)
    print(f"round trip on S3: hit, backface, rejected, none {host.counts[0].tolist()}; start {d0[1] * 1000:.2f} mm + {np.degrees(d0[2]):.3f} deg, "
          f"after relocalize {d1[1] * 1000:.2f} mm + {np.degrees(d1[2]):.3f} deg, loss {hist[0]:.3e} -> {hist[-1]:.3e}")
    assert ok and d1[0] < d0[0], (d0, d1)
    kf.close()


def test_save_view_pgm(dev, scene, tmp_path):
    torch, capi, pl = dev
    a, prm = scene["a"], scene["prm"]
    shade = a.render_views(scene["poses"][:1], intr=small_intr(prm), size=SIZE, outputs=("shade",)).shade[0]
    assert shade.any()
    path = str(tmp_path / "view.pgm")
    pl.save_view_pgm(path, shade)
    raw = open(path, "rb").read()
    head = b"P5\n%d %d\n255\n" % (SIZE[1], SIZE[0])
    assert raw.startswith(head) and len(raw) == len(head) + SIZE[0] * SIZE[1] and raw[len(head):] == shade.tobytes()
    on_device = a.render_views(scene["poses"][:1], intr=small_intr(prm), size=SIZE, outputs=("shade",), device=True).shade[0]
    pl.save_view_pgm(path, on_device)
    assert open(path, "rb").read() == raw
    with pytest.raises(ValueError):
        pl.save_view_pgm(path, np.zeros((2, 3), np.float32))


def test_shard_mode_refuses(dev, scene, tmp_path):
    """Two ranks as threads on one GPU: the three calls raise XsError (-2) on every rank and do nothing, and the pipeline tracks the next frame."""
    torch, capi, pl = dev
    sh = importlib.import_module("x-slam_amd.sharded")
    a, frames, poses = scene["a"], scene["frames"], scene["poses"]
    path = str(tmp_path / "a.ckpt")
    a.save_checkpoint(path)
    world = 2
    prm = dict(synth.s1_params(N), icp_shard_rows=False)
    lw = sh.LocalWorld(torch, world)
    shards = [sh.ShardedKinectFusion(prm, r, world, collective=lw.collective_for(r)) for r in range(world)]
    refused, codes, errors = [0] * world, [None] * world, []

    def work(r):
        try:
            assert shards[r].process_frame(frames[0]) == 1
            for call in (lambda: shards[r].render_views(poses), lambda: shards[r].render_map(a, poses), lambda: shards[r].render_checkpoint(path, poses)):
                try:
                    call()
                except capi.XsError:
                    refused[r] += 1
            m = np.ascontiguousarray(poses[:1], np.float32).reshape(-1)
            out = np.zeros(4, np.uint32)
            codes[r] = pl._lib.xs_kf_render_views(shards[r].h, 1, m.ctypes.data_as(pl._f32p), 1, None, 8, 8, None, None, None, None, None, out.ctypes.data, 0)
            assert shards[r].process_frame(frames[1]) == 1
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            lw.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert refused == [3] * world and codes == [-2] * world
    for s in shards:
        s.close()
