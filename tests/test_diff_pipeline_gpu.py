"""GPU: map differencing at the orchestrator's level (KinectFusion.diff_map, diff_checkpoint, xs_kf_diff_volume) at 64^3
on the synthetic scene S1, six frames, as tests/test_merge_pipeline_gpu.py.  The masks are compared for equality with the numpy model of
tests/diff_cases.py on the downloaded volumes, the records with the scipy cluster model on those masks; nothing a call touches may change."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest
from scipy import ndimage

import diff_cases as dc
import frontier_cases as fc
import merge_cases as mc
from helpers import synth

pytestmark = pytest.mark.gpu
N, FRAMES = 64, 6
BALL_R = 1.5                 # voxels: after six frames at 64^3 the largest cube of observed free space has five voxels a side
PATCH_HALF = 5               # the patch is a cube of 2 * PATCH_HALF + 1 voxels


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


def cube(vol):
    return tuple(a.reshape(N, N, N) for a in vol)


def same_volume(x, y):
    return mc.same_bits(x[0], y[0]) and np.array_equal(x[1], y[1]) and mc.same_bits(x[2], y[2])


def edited(vol, tranc_vox):
    """A's arrays with two edits, and where they are: a ball of analytic TSDF min-ed into a cube of observed free space (weight >= 1, value 1:
    something that appeared in the copy), and a patch of A's surface band overwritten with value 1 (something that went away in the copy)."""
    v, w, g = (a.copy() for a in cube(vol))
    free = (w >= 1) & (v == 1.0)
    half = int(np.ceil(BALL_R))
    # a centre whose cube of 2 * half + 1 voxels is observed free throughout, at least half + 1 voxels from the faces
    whole = ndimage.minimum_filter(free.astype(np.uint8), size=2 * half + 1, mode="constant", cval=0).astype(bool)
    whole[:half + 1] = whole[-half - 1:] = False
    whole[:, :half + 1] = whole[:, -half - 1:] = False
    whole[:, :, :half + 1] = whole[:, :, -half - 1:] = False
    zs, ys, xs = np.nonzero(whole)
    assert len(zs) > 0, "no cube of observed free space for the ball"
    k = len(zs) // 2
    centre = np.array([xs[k], ys[k], zs[k]])
    zz, yy, xx = np.meshgrid(np.arange(N), np.arange(N), np.arange(N), indexing="ij")
    dist = np.sqrt(((xx - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (zz - centre[2]) ** 2).astype(np.float64))
    ball = np.clip((dist - BALL_R) / tranc_vox, -1.0, 1.0).astype(np.float32)
    box = (np.abs(xx - centre[0]) <= half) & (np.abs(yy - centre[1]) <= half) & (np.abs(zz - centre[2]) <= half)
    assert free[box].all()
    v[box] = np.minimum(v[box], ball[box])
    # the patch: around a voxel of matter (value < 0 with weight), the band inside it set to free
    mz, my, mx = np.nonzero((cube(vol)[0] < 0) & (w >= 1))
    assert len(mz) > 100
    j = len(mz) // 2
    pc = np.array([mx[j], my[j], mz[j]])
    patch = (np.abs(xx - pc[0]) <= PATCH_HALF) & (np.abs(yy - pc[1]) <= PATCH_HALF) & (np.abs(zz - pc[2]) <= PATCH_HALF)
    band = patch & (w >= 1) & (np.abs(cube(vol)[0]) < 1)
    assert not (band & box).any()
    v[band] = np.float32(1.0)
    return (v, w, g), dict(centre=centre, half=half, ball_inside=(dist < BALL_R), patch=patch, patch_centre=pc)


@pytest.fixture(scope="module")
def scene(dev):
    """A after six frames (never modified by a test), its edited copy as torch arrays and as the map of a second instance B."""
    torch, capi, pl = dev
    prm = synth.s1_params(N)
    frames = [torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda() for k in range(FRAMES + 1)]
    a = pl.KinectFusion(prm)
    for k in range(FRAMES):
        assert a.process_frame(frames[k]) == 1
    a.synchronize()
    volume = tuple(x.copy() for x in a.volume())
    vs = float(np.float32(prm["tsdf_voxel_size"]))
    src_host, where = edited(volume, a.tranc_dist() / vs)
    src = tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in src_host)
    b = pl.KinectFusion(prm)          # B: a fresh instance that merged the edited copy under the identity: the copy where it carries weight
    n = C.c_ulonglong(0)
    eye = np.eye(4)
    res = np.array([N, N, N], np.int32)
    assert pl._lib.xs_kf_merge_volume(b.h, src[0].data_ptr(), src[1].data_ptr(), src[2].data_ptr(), N * 4, res.ctypes.data_as(pl._i32p), vs, a.tranc_dist(),
                                      eye.ctypes.data_as(pl._f64p), 1, C.byref(n)) == 1
    yield dict(a=a, b=b, prm=prm, frames=frames, volume=volume, src=src, src_host=src_host, where=where, vs=vs)
    a.close()
    b.close()


def diff_volume(pl, kf, src, T, vs, tranc, min_weight=1, lo=0.0, hi=0.5, cell=0, min_size=1, capacity=4096, masks=True):
    """xs_kf_diff_volume: (rc, this records, other records, counts, masks or None)."""
    u64p, res = C.POINTER(C.c_uint64), np.array([N, N, N], np.int32)
    recs = [np.zeros((max(capacity, 1), 8), np.uint64) for _ in range(2)]
    nt, no, counts = C.c_int(-7), C.c_int(-7), np.zeros(3, np.uint64)
    dense = [np.full((N, N, N), 0x77, np.uint8) for _ in range(2)] if masks else None
    dp = [d.ctypes.data_as(C.POINTER(C.c_ubyte)) for d in dense] if masks else [None, None]
    t = np.ascontiguousarray(T, np.float64)
    rc = pl._lib.xs_kf_diff_volume(kf.h, src[0].data_ptr(), src[1].data_ptr(), N * 4, res.ctypes.data_as(pl._i32p), vs, tranc, t.ctypes.data_as(pl._f64p),
                                   min_weight, lo, hi, cell, min_size, capacity, recs[0].ctypes.data_as(u64p), C.byref(nt), recs[1].ctypes.data_as(u64p),
                                   C.byref(no), counts.ctypes.data_as(C.POINTER(C.c_ulonglong)), dp[0], dp[1])
    return rc, recs[0][:max(nt.value, 0)], recs[1][:max(no.value, 0)], tuple(int(c) for c in counts), dense, (nt.value, no.value)


def same_records(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()


def test_self_diff_is_empty(dev, scene):
    """A against a fresh instance that merged A under the identity: no cluster, nothing in either class, every voxel with weight compared."""
    torch, capi, pl = dev
    a, prm = scene["a"], scene["prm"]
    copy = pl.KinectFusion(prm)
    copy.merge_map(a)
    assert same_volume(copy.volume(), scene["volume"])
    d = a.diff_map(copy, min_size=1, masks=True)
    assert isinstance(d, pl.MapDiff)
    assert d.counts == dict(compared=int((scene["volume"][1] >= 1).sum()), only_this=0, only_other=0) and d.counts["compared"] > 1000
    assert len(d.only_this) == 0 and len(d.only_other) == 0 and d.only_this.dtype == pl.KinectFusion.FRONTIER_DTYPE
    assert d.masks[0].shape == (N, N, N) and d.masks[0].dtype == np.uint8 and not d.masks[0].any() and not d.masks[1].any()
    assert a.diff_map(copy).masks is None
    copy.close()


def test_edited_source(dev, scene):
    """xs_kf_diff_volume of A against its edited copy: the masks are the numpy model's on the same arrays, the ball is the largest only_other
    cluster, the only_this clusters lie inside the patch."""
    torch, capi, pl = dev
    a, where, vs = scene["a"], scene["where"], scene["vs"]
    this, other = cube(scene["volume"]), scene["src_host"]
    rc, rt, ro, counts, dense, _ = diff_volume(pl, a, scene["src"], np.eye(4), vs, a.tranc_dist())
    assert rc == 1
    mt, mo, mcounts = dc.diff(this, other, mc.xform(), 1)
    print("counts", counts, mcounts, "clusters", len(rt), len(ro))
    assert counts == mcounts and mcounts[1] > 0 and mcounts[2] > 0
    assert np.array_equal(dense[0], mt.astype(np.uint8)) and np.array_equal(dense[1], mo.astype(np.uint8))
    assert np.array_equal(rt, dc.clusters(mt, 0)) and np.array_equal(ro, dc.clusters(mo, 0))
    # what appeared in the copy: the ball's interior, whole (it lies in observed free space), and nothing else
    assert np.array_equal(mo, where["ball_inside"])
    big = ro[np.argmax(ro[:, 1])]
    lo_box, hi_box = np.array(fc.unpack_box(big[5])), np.array(fc.unpack_box(big[6]))
    c, h = where["centre"], where["half"]
    assert (lo_box >= c - h - 1).all() and (hi_box <= c + h + 1).all()
    centroid = big[2:5].astype(np.float64) / float(big[1])
    assert np.abs(centroid - c).max() <= 1.0 and int(big[1]) == int(where["ball_inside"].sum())
    # what went away in the copy: inside the patch
    assert mt[where["patch"]].sum() == mt.sum()
    pc = where["patch_centre"]
    for r in rt:
        assert (np.array(fc.unpack_box(r[5])) >= pc - PATCH_HALF).all() and (np.array(fc.unpack_box(r[6])) <= pc + PATCH_HALF).all()
    # cells and min_size: the model's records again
    rc, rt8, ro8, _, _, _ = diff_volume(pl, a, scene["src"], np.eye(4), vs, a.tranc_dist(), cell=8, min_size=3, masks=False)
    assert rc == 1 and np.array_equal(rt8, dc.select(dc.clusters(mt, 8), 3)) and np.array_equal(ro8, dc.select(dc.clusters(mo, 8), 3))
    # and through Python: the same records, converted as frontiers() converts them
    d = a.diff_map(scene["b"], min_size=1)
    assert d.counts == dict(compared=mcounts[0], only_this=mcounts[1], only_other=mcounts[2])
    assert np.array_equal(d.only_other["label"], ro[:, 0].astype(np.uint32)) and np.array_equal(d.only_other["count"], ro[:, 1])
    assert np.array_equal(d.only_other["min"][np.argmax(ro[:, 1])], lo_box) and np.array_equal(d.only_other["max"][np.argmax(ro[:, 1])], hi_box)
    want_centroid = np.stack([fc.centroid(r, vs) for r in rt])
    assert np.array_equal(d.only_this["centroid"], want_centroid) and np.array_equal(d.only_this["sum"], rt[:, 2:5])


def test_swapping_the_maps_swaps_the_lists(dev, scene):
    torch, capi, pl = dev
    a, b = scene["a"], scene["b"]
    ab, ba = a.diff_map(b, min_size=1, masks=True), b.diff_map(a, min_size=1, masks=True)
    assert len(ab.only_this) > 0 and len(ab.only_other) > 0
    assert same_records(ab.only_this, ba.only_other) and same_records(ab.only_other, ba.only_this)
    assert ab.counts == dict(compared=ba.counts["compared"], only_this=ba.counts["only_other"], only_other=ba.counts["only_this"])
    assert np.array_equal(ab.masks[0], ba.masks[1]) and np.array_equal(ab.masks[1], ba.masks[0])


def test_checkpoint_equals_map(dev, scene, tmp_path):
    """diff_checkpoint of A's saved checkpoint is diff_map(A), under the identity, a half-voxel shift and a 10 degree rotation; the masks are
    the model's through merge_affine."""
    torch, capi, pl = dev
    a, b, vs = scene["a"], scene["b"], scene["vs"]
    path = str(tmp_path / "a.ckpt")
    a.save_checkpoint(path)
    this, other = cube(b.volume()), cube(scene["volume"])
    shift, rot = np.eye(4), np.eye(4)
    shift[:3, 3] = np.array([0.5, -0.5, 0.5]) * vs
    rot[:3, :3] = mc.rotation((0.2, 1.0, 0.1), np.radians(10.0))
    centre = np.full(3, 0.5 * N * vs)
    rot[:3, 3] = centre - rot[:3, :3] @ centre + np.array([0.3, -0.2, 0.1]) * vs
    for name, T in (("identity", None), ("shift", shift), ("rotation", rot)):
        by_map = b.diff_map(a, T, min_size=2, cell_vox=16, masks=True)
        by_file = b.diff_checkpoint(path, T, min_size=2, cell_vox=16, masks=True)
        assert by_map.counts == by_file.counts and same_records(by_map.only_this, by_file.only_this) and same_records(by_map.only_other, by_file.only_other)
        assert np.array_equal(by_map.masks[0], by_file.masks[0]) and np.array_equal(by_map.masks[1], by_file.masks[1])
        m = pl.merge_affine(np.eye(4) if T is None else T, vs, vs)
        mt, mo, counts = dc.diff(this, other, m, 1)
        print(name, by_map.counts, counts)
        assert by_map.counts == dict(compared=counts[0], only_this=counts[1], only_other=counts[2]) and counts[0] > 1000
        assert np.array_equal(by_map.masks[0], mt.astype(np.uint8)) and np.array_equal(by_map.masks[1], mo.astype(np.uint8))
        for got, mask in ((by_map.only_this, mt), (by_map.only_other, mo)):
            want = dc.select(dc.clusters(mask, 16), 2)
            assert np.array_equal(got["label"], want[:, 0].astype(np.uint32)) and np.array_equal(got["count"], want[:, 1])
    # bad arguments: ValueError, nothing done
    nan = np.eye(4)
    nan[1, 2] = np.nan
    for call in (lambda: b.diff_map(a, nan), lambda: b.diff_map(a, min_weight=0), lambda: b.diff_map(b), lambda: b.diff_map(a, lo=0.5, hi=0.25),
                 lambda: b.diff_map(a, lo=float("nan")), lambda: b.diff_map(a, cell_vox=12), lambda: b.diff_checkpoint(path, nan),
                 lambda: b.diff_checkpoint(str(tmp_path / "missing.ckpt")), lambda: b.diff_checkpoint(path, hi=float("inf"))):
        with pytest.raises(ValueError):
            call()
    other_trunc = pl.KinectFusion(dict(scene["prm"], thres_range=scene["prm"]["thres_range"] + 1))
    with pytest.raises(ValueError):
        b.diff_map(other_trunc)
    other_trunc.close()


def test_nothing_is_modified(dev, scene):
    """Around a call: the volume generation, the volume's bits, frontiers() and the relocalisation of a frame are what they were, on both maps."""
    torch, capi, pl = dev
    a, b, frames = scene["a"], scene["b"], scene["frames"]
    start = a.camera2volume().copy()
    start[0, 3, 0] += 0.01
    before = [(k.volume_generation(), tuple(x.copy() for x in k.volume()), k.frontiers(), k.relocalize(frames[FRAMES], start)) for k in (a, b)]
    assert len(before[0][2]) > 0 and before[0][3][0]
    d = a.diff_map(b, min_size=1, masks=True)
    assert d.counts["only_other"] > 0
    for k, (gen, vol, fr, rl) in zip((a, b), before):
        assert k.volume_generation() == gen and same_volume(k.volume(), vol)
        assert np.array_equal(k.frontiers(), fr)
        again = k.relocalize(frames[FRAMES], start)
        assert again[0] == rl[0] and np.array_equal(again[1].view(np.uint32), rl[1].view(np.uint32)) and np.array_equal(again[2], rl[2])
    assert same_volume(a.volume(), scene["volume"])


def test_a_small_capacity_takes_the_retry(dev, scene):
    """min_size 1, cells of 8 voxels and room for one record fewer than the longer list (and for none): -4 with both needed counts and nothing
    else written; diff_map fetches the lists with a second run."""
    torch, capi, pl = dev
    a, vs = scene["a"], scene["vs"]
    full = diff_volume(pl, a, scene["src"], np.eye(4), vs, a.tranc_dist(), cell=8, masks=False)
    longer = max(len(full[1]), len(full[2]))
    assert full[0] == 1 and min(len(full[1]), len(full[2])) >= 1
    for capacity in sorted({0, longer - 1}):
        rc, rt, ro, counts, dense, needed = diff_volume(pl, a, scene["src"], np.eye(4), vs, a.tranc_dist(), cell=8, capacity=capacity, masks=True)
        assert rc == -4 and needed == (len(full[1]), len(full[2])) and counts == (0, 0, 0), (capacity, rc, needed)
        assert all((d == 0x77).all() for d in dense)
    for capacity in (0, longer - 1, longer):
        d = a.diff_map(scene["b"], min_size=1, cell_vox=8, capacity=capacity)
        assert np.array_equal(d.only_this["label"], full[1][:, 0].astype(np.uint32)) and np.array_equal(d.only_this["count"], full[1][:, 1])
        assert np.array_equal(d.only_other["label"], full[2][:, 0].astype(np.uint32)) and np.array_equal(d.only_other["count"], full[2][:, 1])
        assert d.counts == dict(compared=full[3][0], only_this=full[3][1], only_other=full[3][2])
    assert diff_volume(pl, a, scene["src"], np.eye(4), vs, a.tranc_dist(), capacity=-1, masks=False)[0] == -1


def test_shard_mode_refuses(dev, scene, tmp_path):
    """Two ranks as threads on one GPU: diff_map and diff_checkpoint raise XsError (-2) on every rank and do nothing, and the pipeline tracks
    the next frame afterwards."""
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
            for call in (lambda: shards[r].diff_map(a), lambda: shards[r].diff_checkpoint(path)):
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
    for s in shards:
        s.close()
