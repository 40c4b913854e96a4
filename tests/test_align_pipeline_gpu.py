"""GPU: aligning maps at the orchestrator's level (KinectFusion.align_map, align_checkpoint) at 64^3 on the synthetic
scene S1, a few frames, as tests/test_merge_pipeline_gpu.py does.  A is the map after six frames; B is A merged into an empty instance under
a whole-voxel shift, so B's voxel d holds A's voxel d + shift bit for bit and the residual of A against B at the true transform is exactly 0."""
import importlib
import threading

import numpy as np
import pytest

import align_cases as ac
import merge_cases as mc
from helpers import synth

pytestmark = pytest.mark.gpu
N, FRAMES = 64, 6
SHIFT = (3, -2, 1)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


def cube(vol):
    return tuple(a.reshape(N, N, N) for a in vol)


def state_of(k):
    return (k.frame_id, k.num_poses(), k.camera2volume().tobytes(), k.world2camera().tobytes(), k.volume_generation())


def same_volume(x, y):
    return mc.same_bits(x[0], y[0]) and np.array_equal(x[1], y[1]) and mc.same_bits(x[2], y[2])


@pytest.fixture(scope="module")
def scene(dev):
    """A after six frames and B = A shifted by whole voxels (neither is modified by a test), the true transform from A's frame to B's, the
    start half a voxel and 0.5 degrees off, and the CPU loops of the float32 model and of its twin from that start (computed once)."""
    torch, capi, pl = dev
    prm = synth.s1_params(N)
    vs = float(np.float32(prm["tsdf_voxel_size"]))
    frames = [torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda() for k in range(FRAMES)]
    a = pl.KinectFusion(prm)
    for k in range(FRAMES):
        assert a.process_frame(frames[k]) == 1
    a.synchronize()
    b = pl.KinectFusion(prm)
    into_b = np.eye(4)                       # B's frame -> A's frame: B's voxel d takes A's voxel d + SHIFT
    into_b[:3, 3] = np.array(SHIFT) * vs
    assert np.array_equal(pl.merge_affine(into_b, vs, vs), mc.xform(offset=SHIFT))
    assert b.merge_map(a, into_b) > 1000
    T_true = np.eye(4)                       # A's frame -> B's frame
    T_true[:3, 3] = -np.array(SHIFT) * vs
    va, vb = tuple(x.copy() for x in a.volume()), tuple(x.copy() for x in b.volume())
    state_a, state_b = state_of(a), state_of(b)          # before any alignment
    assert a.relocalization_index_voxels() == 0 and b.relocalization_index_voxels() == 0
    xyz, gt = ac.band_of(cube(va)[0])
    src = (cube(vb)[0], cube(vb)[1])
    T0 = ac.perturbed(T_true, (N, N, N), vs)
    model = ac.loop(xyz, gt, src, T0, vs, vs, 10)
    twin = ac.loop(xyz, gt, src, T0, vs, vs, 10, twin=True)
    yield dict(a=a, b=b, prm=prm, vs=vs, va=va, vb=vb, xyz=xyz, gt=gt, src=src, T_true=T_true, T0=T0, model=model, twin=twin, frames=frames,
               state_a=state_a, state_b=state_b)
    a.close()
    b.close()


def test_converging_to_the_truth(dev, scene):
    """From half a voxel and 0.5 degrees off: ends ok, the loss history never rises, the final T
    is the CPU float32 model's to within four times the model's own distance from its float64 twin, and the final loss is at most the loss of
    an iterations = 0 call at the truth plus the pass bound."""
    torch, capi, pl = dev
    a, b, vs = scene["a"], scene["b"], scene["vs"]
    ok, T, rep, hist = a.align_map(b, scene["T0"], iterations=10)
    m_ok, m_T, m_hist, m_ev = scene["model"]
    t_ok, t_T, t_hist, _ = scene["twin"]
    measured = ac.corner_displacement(m_T, t_T, (N, N, N), vs)
    gpu_model = ac.corner_displacement(T, m_T, (N, N, N), vs)
    ev = ac.evaluate(scene["xyz"], scene["gt"], scene["src"], ac.seeded_maps(T, vs, vs))
    pass_bound = ev["bound"][27] / max(ev["sums32"][28], 1)
    ok0, T_same, rep0, hist0 = a.align_map(b, scene["T_true"], iterations=0)
    print(f"model-twin corner displacement {measured:.3e} m, gpu-model {gpu_model:.3e} m, constant {ac.PIPELINE_MODEL_TWIN_CORNER_M:.3e} m; "
          f"loss history {hist}; loss at truth {hist0}; pass bound {pass_bound:.3e}; counts {rep['count']} / {rep0['count']} / band {rep['band_voxels']}; "
          f"to truth {ac.corner_displacement(T, scene['T_true'], (N, N, N), vs):.3e} m")
    assert m_ok and t_ok and measured <= ac.PIPELINE_MODEL_TWIN_CORNER_M
    assert ok and len(hist) == 11 and rep["start"] == 0 and rep["ended_ok"] == 1 and rep["passes"] == 11 and rep["band_voxels"] == len(scene["gt"])
    assert (np.diff(hist) <= 0).all(), hist
    assert hist[0] > 1e-4 and rep["count"] > 1000 and rep["loss"] == hist[-1] and abs(rep["sum_r2"] / rep["count"] - rep["loss"]) <= 1e-15 * rep["loss"]
    assert gpu_model <= 4 * ac.PIPELINE_MODEL_TWIN_CORNER_M
    assert ok0 and np.array_equal(T_same, scene["T_true"]) and len(hist0) == 1 and rep0["passes"] == 1
    assert hist0[0] <= pass_bound and rep0["count"] > 1000     # B holds A's own numbers: 0 but for products of two imaginary parts
    assert hist[-1] <= hist0[0] + pass_bound
    assert ac.corner_displacement(T, scene["T_true"], (N, N, N), vs) < 0.01 * vs


def test_multi_start(dev, scene):
    """Three starts, one of them hopeless (the maps do not overlap): the winner is the best start by S = count - sum r^2, the report says so,
    and it is what that start gives alone."""
    torch, capi, pl = dev
    a, b, vs = scene["a"], scene["b"], scene["vs"]
    hopeless = scene["T_true"].copy()
    hopeless[:3, 3] += 70 * vs
    rough = ac.perturbed(scene["T_true"], (N, N, N), vs, shift_voxels=(0.9, 0.6, -0.8), degrees=1.0)
    starts = np.stack([hopeless, rough, scene["T0"]])
    ok, T, rep, hist = a.align_map(b, starts, iterations=6)
    alone = [a.align_map(b, s, iterations=6) for s in starts]
    assert not alone[0][0] and alone[0][2]["start"] == -1 and np.array_equal(alone[0][1], hopeless) and len(alone[0][3]) == 0
    S = [r[2]["count"] - r[2]["sum_r2"] if r[0] else -np.inf for r in alone]
    best = int(np.argmax(S))
    assert best in (1, 2)
    assert ok and rep["start"] == best and rep["ended_ok"] == 2 and rep["passes"] == 7
    assert np.array_equal(T, alone[best][1]) and np.array_equal(hist, alone[best][3]) and rep["count"] == alone[best][2]["count"]
    assert rep["sum_r2"] == alone[best][2]["sum_r2"]


def test_merging_under_the_aligned_transform(dev, scene):
    """A copy of A merged with B under the aligned T agrees with B (iterations = 0 loss at the aligned T) no worse than the copy merged
    under the start."""
    torch, capi, pl = dev
    a, b, prm = scene["a"], scene["b"], scene["prm"]
    ok, T, rep, hist = a.align_map(b, scene["T0"])
    assert ok
    losses = []
    for Tm in (T, scene["T0"]):
        c = pl.KinectFusion(prm)
        c.merge_map(a)
        assert same_volume(c.volume(), scene["va"])
        assert c.merge_map(b, Tm) > 1000
        ok_c, _, rep_c, hist_c = c.align_map(b, T, iterations=0)
        assert ok_c and rep_c["count"] > 1000
        losses.append(hist_c[0])
        c.close()
    assert losses[0] <= losses[1] and losses[1] > 0


def test_align_checkpoint_equals_align_map(dev, scene, tmp_path):
    torch, capi, pl = dev
    a, b = scene["a"], scene["b"]
    path = str(tmp_path / "b.ckpt")
    b.save_checkpoint(path)
    starts = np.stack([scene["T0"], scene["T_true"]])
    by_map, by_file = a.align_map(b, starts, iterations=4), a.align_checkpoint(path, starts, iterations=4)
    assert by_map[0] and by_file[0] and np.array_equal(by_map[1].view(np.uint64), by_file[1].view(np.uint64))
    assert by_map[2] == by_file[2] and np.array_equal(by_map[3].view(np.uint64), by_file[3].view(np.uint64))
    raw = open(path, "rb").read()
    for name, blob in {"truncated": raw[:-4], "magic": b"XSTSDF1\0" + raw[8:]}.items():
        p = str(tmp_path / (name + ".ckpt"))
        open(p, "wb").write(blob)
        with pytest.raises(ValueError):
            a.align_checkpoint(p, scene["T0"])
    with pytest.raises(ValueError):
        a.align_checkpoint(str(tmp_path / "missing.ckpt"), scene["T0"])


def test_nothing_is_modified(dev, scene):
    """Against the state the fixture recorded before any alignment: volumes, frame numbers, poses and the volume generation (what the band
    index and every other cached map are keyed by) of both instances are what they were; the other map's band index is never built, this
    map's is built once from the unchanged volume; a second call gives the same bits."""
    torch, capi, pl = dev
    a, b = scene["a"], scene["b"]
    first = a.align_map(b, scene["T0"], iterations=3)
    second = a.align_map(b, scene["T0"], iterations=3)
    a.align_map(b, scene["T_true"], iterations=0)
    assert state_of(a) == scene["state_a"] and state_of(b) == scene["state_b"]
    assert a.relocalization_index_voxels() == len(scene["gt"]) and b.relocalization_index_voxels() == 0
    assert same_volume(a.volume(), scene["va"]) and same_volume(b.volume(), scene["vb"])
    assert np.array_equal(first[1].view(np.uint64), second[1].view(np.uint64)) and np.array_equal(first[3].view(np.uint64), second[3].view(np.uint64))
    assert first[2] == second[2]


def test_a_start_that_keeps_nothing_does_not_win(dev, scene):
    """iterations = 0 has only the loss pass: a start that misses the other map keeps no voxel and must not end ok, alone or beside a
    start that fits; the report counts only the starts that kept six voxels."""
    torch, capi, pl = dev
    a, b, vs = scene["a"], scene["b"], scene["vs"]
    miss = scene["T_true"].copy()
    miss[:3, 3] += 70 * vs
    ok, T, rep, hist = a.align_map(b, miss, iterations=0)
    assert not ok and rep["start"] == -1 and rep["ended_ok"] == 0 and rep["passes"] == 1 and np.array_equal(T, miss) and len(hist) == 0
    ok, T, rep, hist = a.align_map(b, np.stack([miss, scene["T_true"]]), iterations=0)
    assert ok and rep["start"] == 1 and rep["ended_ok"] == 1 and rep["count"] > 1000 and np.array_equal(T, scene["T_true"])


def test_refusals(dev, scene):
    """ValueError, nothing done: another truncation distance, a T that is not finite, the instance itself as source, arguments out of range."""
    torch, capi, pl = dev
    a, b, prm = scene["a"], scene["b"], scene["prm"]
    nan = np.eye(4)
    nan[1, 2] = np.nan
    stack = np.stack([np.eye(4), nan])
    other = pl.KinectFusion(dict(prm, thres_range=prm["thres_range"] + 1))
    assert other.tranc_dist() != a.tranc_dist()
    for call in (lambda: a.align_map(other), lambda: a.align_map(b, nan), lambda: a.align_map(b, stack), lambda: a.align_map(a),
                 lambda: a.align_map(b, iterations=-1), lambda: a.align_map(b, min_weight=0), lambda: a.align_map(b, max_residual=0.0),
                 lambda: a.align_map(b, max_residual=float("nan")), lambda: a.align_map(b, damping=-1.0)):
        with pytest.raises(ValueError):
            call()
    other.close()
    assert same_volume(a.volume(), scene["va"]) and same_volume(b.volume(), scene["vb"])


def test_shard_mode_refuses(dev, scene, tmp_path):
    """Two ranks as threads on one GPU: align_map and align_checkpoint raise XsError (-2) on every rank, and the pipeline tracks the next
    frame afterwards."""
    torch, capi, pl = dev
    sh = importlib.import_module("x-slam_amd.sharded")
    b, frames = scene["b"], scene["frames"]
    path = str(tmp_path / "b.ckpt")
    b.save_checkpoint(path)
    world = 2
    prm = dict(scene["prm"], icp_shard_rows=False)
    lw = sh.LocalWorld(torch, world)
    shards = [sh.ShardedKinectFusion(prm, r, world, collective=lw.collective_for(r)) for r in range(world)]
    refused, errors = [0] * world, []

    def work(r):
        try:
            assert shards[r].process_frame(frames[0]) == 1
            for call in (lambda: shards[r].align_map(b), lambda: shards[r].align_checkpoint(path)):
                try:
                    call()
                except capi.XsError:
                    refused[r] += 1
            assert shards[r].process_frame(frames[1]) == 1
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            lw.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert refused == [2] * world
    for s in shards:
        s.close()
