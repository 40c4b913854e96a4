"""GPU: merging maps at the orchestrator's level (KinectFusion.merge_map, merge_checkpoint) at 64^3 on the synthetic
scene S1, a few frames, as the pipeline_s1_n64 fixture's test does.  Volumes are compared for equal bits, and everything derived from the
volume (point cloud, mesh over the rebuilt sign map, relocalisation over the rebuilt band index, frontiers) must follow the merged volume."""
import importlib
import struct
import threading

import numpy as np
import pytest

import merge_cases as mc
from helpers import synth

pytestmark = pytest.mark.gpu
N, FRAMES = 64, 6


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


@pytest.fixture(scope="module")
def scene(dev):
    """A after six frames (never modified by a test), the frames, the parameters."""
    torch, capi, pl = dev
    prm = synth.s1_params(N)
    frames = [torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda() for k in range(FRAMES + 1)]
    a = pl.KinectFusion(prm)
    for k in range(FRAMES):
        assert a.process_frame(frames[k]) == 1
    a.synchronize()
    yield dict(a=a, prm=prm, frames=frames, volume=tuple(x.copy() for x in a.volume()))
    a.close()


def same_volume(x, y):
    return mc.same_bits(x[0], y[0]) and np.array_equal(x[1], y[1]) and mc.same_bits(x[2], y[2])


def cube(vol):
    return tuple(a.reshape(N, N, N) for a in vol)


def test_identity_into_a_fresh_instance_is_the_map(dev, scene):
    """C.merge_map(A): C's volume is A's bit for bit, and the point cloud, the mesh (the rebuilt sign map), relocalisation of a frame (the
    rebuilt band index) and the frontiers of C are A's.  A itself is unchanged."""
    torch, capi, pl = dev
    a, prm, frames = scene["a"], scene["prm"], scene["frames"]
    c = pl.KinectFusion(prm)
    poses, frame_id, c2v = c.num_poses(), c.frame_id, c.camera2volume().copy()
    written = c.merge_map(a)
    assert written == int((scene["volume"][1] >= 1).sum()) > 1000
    assert same_volume(c.volume(), scene["volume"]) and same_volume(a.volume(), scene["volume"])
    assert (c.num_poses(), c.frame_id) == (poses, frame_id) and np.array_equal(c.camera2volume(), c2v)
    pa, pc = a.export_point_cloud(), c.export_point_cloud()
    assert len(pa[0]) > 100 and mc.same_bits(pa[0], pc[0]) and np.array_equal(pa[1].view(np.uint32), pc[1].view(np.uint32))
    ma, mcm = a.export_mesh(), c.export_mesh()
    assert len(ma.triangles) > 100 and mc.same_bits(ma.vertices, mcm.vertices) and np.array_equal(ma.triangles, mcm.triangles)
    assert np.array_equal(ma.edge_keys, mcm.edge_keys) and np.array_equal(ma.normals.view(np.uint32), mcm.normals.view(np.uint32))
    start = a.camera2volume().copy()
    start[0, 3, 0] += 0.01
    ra, rc = a.relocalize(frames[FRAMES], start), c.relocalize(frames[FRAMES], start)
    assert ra[0] and rc[0] and np.array_equal(ra[1].view(np.uint32), rc[1].view(np.uint32)) and np.array_equal(ra[2], rc[2])
    fa, fcc = a.frontiers(), c.frontiers()
    assert len(fa) > 0 and np.array_equal(fa, fcc)
    # a second merge of the same map doubles the weights and leaves the values where two equal observations leave them
    c.merge_map(a)
    v, w, g = c.volume()
    assert np.array_equal(w, np.minimum(2 * scene["volume"][1], prm["max_integration_weight"]))
    c.close()


def test_shift_by_whole_voxels_is_a_slice(dev, scene):
    """T a translation by (3, -2, 5) voxel edges: C's voxel d holds A's voxel d + (3, -2, 5) where that exists and carries weight, zero elsewhere."""
    torch, capi, pl = dev
    a, prm = scene["a"], scene["prm"]
    vs = float(np.float32(prm["tsdf_voxel_size"]))
    T = np.eye(4)
    T[:3, 3] = np.array([3, -2, 5]) * vs
    assert np.array_equal(pl.merge_affine(T, vs, vs), mc.xform(offset=(3, -2, 5)))
    c = pl.KinectFusion(prm)
    written = c.merge_map(a, T)
    av, aw, ag = cube(scene["volume"])
    want = [np.zeros_like(x) for x in (av, aw, ag)]
    for dst, src in zip(want, (av, aw, ag)):
        dst[:N - 5, 2:, :N - 3] = src[5:, :N - 2, 3:]                     # [z, y, x]: z + 5, y - 2, x + 3
    keep = want[1] >= 1
    for k in (0, 2):
        want[k] = np.where(keep, want[k], np.float32(0))
    assert written == int(keep.sum()) > 1000
    assert same_volume(cube(c.volume()), want)
    c.close()


def test_merging_a_twin_doubles_the_weights(dev, scene):
    """A1 and A2 process the same frames; A1.merge_map(A2): weights are min(2 w, max) exactly, values and grads the numpy model's on the two
    downloaded volumes, the next frame is tracked and the camera stays within a voxel edge of the twin's."""
    torch, capi, pl = dev
    prm, frames = scene["prm"], scene["frames"]
    a1, a2 = pl.KinectFusion(prm), pl.KinectFusion(prm)
    for k in range(FRAMES):
        assert a1.process_frame(frames[k]) == 1 and a2.process_frame(frames[k]) == 1
    v1, v2 = a1.volume(), a2.volume()
    assert same_volume(v1, v2) and same_volume(v1, scene["volume"])
    poses, frame_id, c2v = a1.num_poses(), a1.frame_id, a1.camera2volume().copy()
    written = a1.merge_map(a2)
    want = mc.merge(cube(v1), cube(v2), mc.xform(), 1, max_weight=int(prm["max_integration_weight"]))
    got = cube(a1.volume())
    assert written == want[3] == int((v2[1] >= 1).sum())
    assert np.array_equal(got[1], np.minimum(2 * cube(v1)[1], int(prm["max_integration_weight"]))) and same_volume(got, want)
    assert (a1.num_poses(), a1.frame_id) == (poses, frame_id) and np.array_equal(a1.camera2volume(), c2v)
    assert a1.process_frame(frames[FRAMES]) == 1 and a2.process_frame(frames[FRAMES]) == 1
    p1, p2 = a1.camera2volume()[:3, 3, 0], a2.camera2volume()[:3, 3, 0]
    assert np.linalg.norm(p1.astype(np.float64) - p2) < prm["tsdf_voxel_size"]
    a1.close()
    a2.close()


def test_merge_checkpoint(dev, scene, tmp_path):
    """save_checkpoint on A then C.merge_checkpoint: the volume merge_map(A) gives.  A truncated file, a wrong magic, trailing bytes and
    another truncation distance return -1 and leave the volume's bits alone; so do bad arguments of merge_map."""
    torch, capi, pl = dev
    a, prm = scene["a"], scene["prm"]
    path = str(tmp_path / "a.ckpt")
    a.save_checkpoint(path)
    c = pl.KinectFusion(prm)
    T = np.eye(4)
    T[:3, :3] = mc.rotation((0.2, 1.0, 0.1), np.radians(10.0))
    T[:3, 3] = (0.3, -0.1, 0.2)
    by_map = c.merge_map(a, T, min_weight=2)
    want = c.volume()
    c.close()
    c = pl.KinectFusion(prm)
    assert c.merge_checkpoint(path, T, min_weight=2) == by_map > 1000
    assert same_volume(c.volume(), want) and not same_volume(want, scene["volume"])
    before = tuple(x.copy() for x in c.volume())
    raw = open(path, "rb").read()
    bad = {"truncated": raw[:-4], "trailing": raw + b"\0\0\0\0", "magic": b"XSTSDF1\0" + raw[8:], "short": raw[:20],
           "tranc": raw[:24] + struct.pack("<f", struct.unpack("<f", raw[24:28])[0] * 2) + raw[28:],
           "sharded": raw[:44] + struct.pack("<ii", 0, 2) + raw[52:]}
    assert struct.unpack("<f", raw[24:28])[0] == c.tranc_dist() and struct.unpack("<ii", raw[44:52]) == (0, 1)
    import ctypes as C
    eye = np.eye(4)
    for name, blob in bad.items():
        p = str(tmp_path / (name + ".ckpt"))
        open(p, "wb").write(blob)
        n = C.c_ulonglong(7)
        assert pl._lib.xs_kf_merge_checkpoint(c.h, p.encode(), eye.ctypes.data_as(pl._f64p), 1, C.byref(n)) == -1, name
        with pytest.raises(ValueError):
            c.merge_checkpoint(p)
    with pytest.raises(ValueError):
        c.merge_checkpoint(str(tmp_path / "missing.ckpt"))
    nan = np.eye(4)
    nan[1, 2] = np.nan
    for call in (lambda: c.merge_checkpoint(path, nan), lambda: c.merge_checkpoint(path, min_weight=0), lambda: c.merge_map(a, nan),
                 lambda: c.merge_map(a, min_weight=0), lambda: c.merge_map(c)):
        with pytest.raises(ValueError):
            call()
    other = pl.KinectFusion(dict(prm, thres_range=prm["thres_range"] + 1))       # another truncation distance
    assert other.tranc_dist() != c.tranc_dist()
    with pytest.raises(ValueError):
        c.merge_map(other)
    other.close()
    assert same_volume(c.volume(), before)
    c.close()


def test_shard_mode_refuses(dev, scene, tmp_path):
    """Two ranks as threads on one GPU: merge_map and merge_checkpoint raise XsError (-2) on every rank and do nothing, and the pipeline
    tracks the next frame afterwards."""
    torch, capi, pl = dev
    sh = importlib.import_module("x-slam_amd.sharded")
    a, frames = scene["a"], scene["frames"]
    path = str(tmp_path / "a.ckpt")
    a.save_checkpoint(path)
    world = 2
    prm = dict(scene["prm"], icp_shard_rows=False)
    lw = sh.LocalWorld(torch, world)
    shards = [sh.ShardedKinectFusion(prm, r, world, collective=lw.collective_for(r)) for r in range(world)]
    refused, errors, same = [0] * world, [], [False] * world

    def work(r):
        try:
            assert shards[r].process_frame(frames[0]) == 1
            before = tuple(x.copy() for x in shards[r].volume())
            for call in (lambda: shards[r].merge_map(a), lambda: shards[r].merge_checkpoint(path)):
                try:
                    call()
                except capi.XsError:
                    refused[r] += 1
            same[r] = same_volume(shards[r].volume(), before)
            assert shards[r].process_frame(frames[1]) == 1
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            lw.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert refused == [2] * world and same == [True] * world
    assert np.array_equal(shards[0].world2camera(), shards[1].world2camera())
    for s in shards:
        s.close()
