"""GPU: scoring many transforms of a point cloud and registering a cloud with no starting guess at the orchestrator's level
(KinectFusion.score_point_transforms, register_points_global and their _map / _checkpoint forms, register_and_fuse(global_search=True);
DESIGN.md section 4.32) on the analytic fixture of tests/align_score_cases.py: an instance at 48^3, voxel 0.1 m, truncation 0.3 m, whose volume
is written through volume_ptr, and the deterministic surface cloud of tests/register_score_cases.py handed over moved by a rotation of 100 or
170 degrees about an axis through the volume's centre plus a shift."""
import ctypes as C
import importlib
import threading

import numpy as np
import pytest

import align_cases as ac
import align_score_cases as asc
import merge_cases as mc
import register_cases as rg
import register_score_cases as rs
from helpers import synth
from test_align_global_pipeline_gpu import params, same_volume, state_of, write_volume
from test_register_gpu import Guarded

pytestmark = pytest.mark.gpu
N, VS = asc.SCENE_N, asc.SCENE_VS
RES = (N, N, N)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


@pytest.fixture(scope="module")
def scene(dev):
    """A (the scene) and E (an instance whose map stays empty; neither is modified by a test), A's volume and both states before any call, the
    clouds, and register_points from the truth itself for each cloud: the minimum the search has to reach (computed once)."""
    torch, capi, pl = dev
    prm = params()
    a, e = pl.KinectFusion(prm), pl.KinectFusion(prm)
    assert abs(a.tranc_dist() - asc.SCENE_TRUNC) < 1e-6
    write_volume(torch, a, *asc.scene_volume())
    va, ve = tuple(x.copy() for x in a.volume()), tuple(x.copy() for x in e.volume())
    states = {"a": state_of(a), "e": state_of(e)}
    assert a.relocalization_index_voxels() == 0 and e.relocalization_index_voxels() == 0
    clouds = {(100, False): rs.handed_cloud(100), (170, False): rs.handed_cloud(170), (100, True): rs.handed_cloud(100, True)}
    assert len(clouds[(100, False)][0]) == rs.SCENE_CLOUD_POINTS and len(clouds[(100, True)][0]) == rs.SCENE_HALF_POINTS
    ref = {k: a.register_points(c, T, iterations=10) for k, (c, T) in clouds.items()}
    yield dict(a=a, e=e, prm=prm, va=va, ve=ve, states=states, clouds=clouds, ref=ref)
    a.close()
    e.close()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def test_score_point_transforms_equals_the_kernel_call(dev, scene):
    """4 101 transforms go through the chunking: every pair is, bit for bit, what xs_tsdf_score_points gives on the downloaded volume (laid out
    with another pitch); strides 1 and 4; the truth, planted at index 7, has the highest S, and its pair is the model's."""
    torch, capi, pl = dev
    a, va = scene["a"], scene["va"]
    cloud, T_true = scene["clouds"][(100, False)]
    vol = (va[0].reshape(N, N, N), va[1].reshape(N, N, N))
    devvol = ac.DevSource(torch, vol, N * 4 + 4)
    devvol.res = list(RES)
    pts = Guarded(len(cloud) * 12, cloud)
    case = rs.scene_case()
    runner = rs.ScoreRunner(torch, capi)
    for stride in (4, 1):
        Ts = pl.transform_candidates_free(4101, pl.points_centroid(cloud, stride), rs.map_band_centroid(vol[0], VS, pl), 0.3)
        Ts[7] = T_true
        xforms = np.stack([rg.xform12_of(T) for T in Ts])
        got = a.score_point_transforms(cloud, Ts, stride=stride)
        assert got.shape == (4101, 2) and got.dtype == np.float64
        want = np.concatenate([runner.run(len(cloud), pts.addr, devvol, case, xforms[:4096], stride), runner.run(len(cloud), pts.addr, devvol, case, xforms[4096:], stride)])
        assert np.array_equal(bits(got), bits(want)), stride
        S = got[:, 1] - got[:, 0]
        assert int(np.argmax(S)) == 7 and got[7, 1] >= 0.99 * -(-len(cloud) // stride)
        rs.check(got[7], rs.score_model(case, xforms[7], stride, pts=cloud), ("truth", stride))
    assert devvol.untouched() and pts.untouched() and runner.tickets_zero()


@pytest.mark.parametrize("deg,half", [(100, False), (170, False), (100, True)], ids=["full_100", "full_170", "half_100"])
def test_search_reaches_the_truth(dev, scene, deg, half):
    """No guess, the defaults (2 048 candidates, stride 4, keep 8, 2 rounds): ends ok, within 0.01 voxel of worst-corner displacement of
    register_points started at the truth in the same run, with at least 0.98 of its S; the report's counts are consistent.  The measured
    distances are printed: DESIGN.md section 4.32 records them.  Measured on an MI355X when this was written: 3.6e-7 m (100 degrees), 3.5e-7 m
    (170 degrees), 6.6e-7 m (the half cloud); the bound is 1e-3 m."""
    torch, capi, pl = dev
    a = scene["a"]
    cloud, T_true = scene["clouds"][(deg, half)]
    r_ok, T_ref, r_rep = scene["ref"][(deg, half)]
    assert r_ok
    S_ref = r_rep["count"] - r_rep["sum_r2"]
    ok, T, rep = a.register_points_global(cloud)
    d = ac.corner_displacement(T, T_ref, RES, VS)
    S = rep["count"] - rep["sum_r2"]
    print(f"{deg} degrees, half {half}: ok {ok}, {d:.3e} m from register_points(truth), S {S:.3f} against {S_ref:.3f}, to the truth {ac.corner_displacement(T, T_true, RES, VS):.3e} m, {rep}")
    assert ok and d <= rs.SEARCH_AGREEMENT_VOXELS * VS and S >= rs.SEARCH_S_FRACTION * S_ref
    assert rep["points"] == len(cloud) and rep["scored_points"] == -(-len(cloud) // 4)
    assert rep["score_launches"] == 3 and 0 <= rep["rank"] < 8 and 1 <= rep["ended_ok"] <= 8 and rep["passes"] >= 11
    assert rep["count"] > 0.9 * len(cloud) and abs(rep["sum_r2"] / rep["count"] - rep["loss"]) <= 1e-15 * rep["loss"]
    assert 0 < rep["S_before"] <= rep["scored_points"] and rep["centroid_distance"] < (1.0 if half else 0.5)
    assert np.array_equal(T[3], [0, 0, 0, 1]) and np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-9


def test_the_identity_start_does_not_get_there(dev, scene):
    """The case the feature exists for: register_points from the identity ends not ok or more than a voxel from the truth."""
    for key in ((100, False), (170, False), (100, True)):
        cloud, T_true = scene["clouds"][key]
        ok, T, rep = scene["a"].register_points(cloud, np.eye(4), iterations=10)
        d = ac.corner_displacement(T, T_true, RES, VS)
        print(f"{key} from the identity: ok {ok}, {d:.3f} m from the truth")
        assert (not ok) or d > VS


def test_sources_and_clouds_give_the_same_bits(dev, scene, tmp_path):
    """The own-map call, the other-instance call and the checkpoint call (dense and sparse) on the same volume, and a host and a device cloud:
    equal transforms and reports, bit for bit; the same for the scoring call.  A second call repeats the first."""
    torch, capi, pl = dev
    a, e = scene["a"], scene["e"]
    cloud, T_true = scene["clouds"][(100, False)]
    own = a.register_points_global(cloud)
    assert own[0]
    dense, sparse = str(tmp_path / "a.ckpt"), str(tmp_path / "a.sparse")
    a.save_checkpoint(dense)
    a.save_checkpoint(sparse, sparse=True)
    on_dev = torch.from_numpy(np.array(cloud)).cuda()
    others = [a.register_points_global(cloud), e.register_map_points_global(a, cloud), e.register_checkpoint_points_global(dense, cloud),
              e.register_checkpoint_points_global(sparse, cloud), a.register_points_global(on_dev), e.register_map_points_global(a, on_dev)]
    for i, r in enumerate(others):
        assert r[0] and np.array_equal(bits(r[1]), bits(own[1])) and r[2] == own[2], i
    Ts = np.stack([T_true, np.eye(4), own[1]])
    want = a.score_point_transforms(cloud, Ts, stride=3)
    for got in (e.score_map_point_transforms(a, cloud, Ts, stride=3), e.score_checkpoint_point_transforms(dense, cloud, Ts, stride=3),
                e.score_checkpoint_point_transforms(sparse, cloud, Ts, stride=3), a.score_point_transforms(on_dev, Ts, stride=3)):
        assert np.array_equal(bits(got), bits(want))
    assert want[0, 1] > 2700 and want[1, 1] < want[0, 1]
    bad = str(tmp_path / "truncated.ckpt")
    open(bad, "wb").write(open(dense, "rb").read()[:-4])
    for call in (lambda: e.register_checkpoint_points_global(bad, cloud), lambda: e.score_checkpoint_point_transforms(bad, cloud, Ts),
                 lambda: e.register_checkpoint_points_global(str(tmp_path / "none.ckpt"), cloud), lambda: e.register_map_points_global(e, cloud)):
        with pytest.raises(ValueError):
            call()


def test_user_candidates(dev, scene):
    """Candidates of the caller's replace the free ones: with the truth among them, no rounds and no iterations, the truth itself comes back."""
    torch, capi, pl = dev
    a = scene["a"]
    cloud, T_true = scene["clouds"][(100, False)]
    Ts = pl.transform_candidates_free(6, pl.points_centroid(cloud, 4), [2.4, 2.4, 2.4], 0.3)
    Ts[3] = T_true
    ok, T, rep = a.register_points_global(cloud, Ts=Ts, rounds=0, iterations=0)
    assert ok and np.array_equal(bits(T), bits(T_true)) and rep["rank"] == 0 and rep["score_launches"] == 1 and rep["passes"] == 1
    pair = a.score_point_transforms(cloud, T_true, stride=4)[0]
    assert rep["S_before"] == pair[1] - pair[0]
    ok, T, rep = a.register_points_global(cloud, Ts=Ts, rounds=0)
    assert ok and ac.corner_displacement(T, scene["ref"][(100, False)][1], RES, VS) <= rs.SEARCH_AGREEMENT_VOXELS * VS


def test_nothing_matches(dev, scene):
    """A map without weight anywhere: not ok, T16_out untouched, at either level; a map with no band voxel: not ok."""
    torch, capi, pl = dev
    cloud, _ = scene["clouds"][(100, False)]
    z = pl.KinectFusion(scene["prm"])
    write_volume(torch, z, asc.scene_volume()[0], np.zeros(RES, np.int32))
    ok, T, rep = z.register_points_global(cloud)
    assert not ok and rep["rank"] == -1 and rep["ended_ok"] == 0 and rep["count"] == 0 and np.array_equal(T, np.eye(4))
    out, report = np.full(16, -7.0), np.zeros(12)
    f64p = C.POINTER(C.c_double)
    assert pl._lib.xs_kf_register_points_global(z.h, len(cloud), cloud.ctypes.data, 0, None, out.ctypes.data_as(f64p), report.ctypes.data_as(f64p)) == 0
    assert (out == -7.0).all() and report[0] == -1 and report[8] == len(cloud) and report[9] == -(-len(cloud) // 4)
    ok, T, rep = scene["e"].register_points_global(cloud)          # no band at all: no centroid, not ok
    assert not ok and rep["rank"] == -1
    z.close()


def test_nothing_is_modified(dev, scene):
    """Against what the fixture recorded before any call: the state tuple, the volumes, volume_generation and the relocalisation index of every
    instance (the map's band centroid comes from buffers of the call's own: no cache is built, this instance's included)."""
    torch, capi, pl = dev
    a, e = scene["a"], scene["e"]
    cloud, _ = scene["clouds"][(100, True)]
    first = a.register_points_global(cloud)
    second = e.register_map_points_global(a, cloud)
    a.score_point_transforms(cloud, np.eye(4))
    assert state_of(a) == scene["states"]["a"] and state_of(e) == scene["states"]["e"]
    assert a.relocalization_index_voxels() == 0 and e.relocalization_index_voxels() == 0
    assert same_volume(a.volume(), scene["va"]) and same_volume(e.volume(), scene["ve"])
    assert first[0] and np.array_equal(bits(first[1]), bits(second[1])) and first[2] == second[2]


def test_register_and_fuse_with_the_search(dev, scene):
    """On a copy of A: with global_search the cloud is fused at the transform register_points_global finds (the same bits as fuse_points at that
    transform on another copy); with the default the call is register_points followed by fuse_points as before, from the identity, which ends
    metres from the truth."""
    torch, capi, pl = dev
    cloud, T_true = scene["clouds"][(100, False)]
    found = scene["a"].register_points_global(cloud)
    copies = []
    for _ in range(2):
        c = pl.KinectFusion(scene["prm"])
        write_volume(torch, c, *asc.scene_volume())
        copies.append(c)
    origin = (T_true[:3, :3].T @ (np.array([2.4, 2.4, 0.5]) - T_true[:3, 3])).astype(np.float32)      # a sensor position, in the cloud's frame
    ok, T, rep, fused = copies[0].register_and_fuse(cloud, origin=origin)
    plain = copies[1].register_points(cloud)
    assert ok == plain[0] and np.array_equal(bits(T), bits(plain[1])) and rep["start"] == plain[2]["start"] and rep["sum_r2"] == plain[2]["sum_r2"]
    assert (fused is None) == (not ok) and ac.corner_displacement(T, T_true, RES, VS) > VS          # (the identity's basin is not the truth's)
    if ok:
        assert copies[1].fuse_points(cloud, plain[1], origin=origin) == fused
    assert same_volume(copies[0].volume(), copies[1].volume())
    for c in copies:
        write_volume(torch, c, *asc.scene_volume())
    ok, T, rep, fused = copies[0].register_and_fuse(cloud, origin=origin, global_search=True)
    assert ok and np.array_equal(bits(T), bits(found[1])) and rep == found[2] and fused["used"] > 0.5 * len(cloud) and fused["written"] > 1000
    want = copies[1].fuse_points(cloud, found[1], origin=origin)
    assert want == fused and same_volume(copies[0].volume(), copies[1].volume())
    for c in copies:
        c.close()


def test_refusals(dev, scene):
    """ValueError, nothing done: options out of range, a wrong struct size, more than 2^24 scored points, candidates that are not finite,
    min_weight 0, clouds of the wrong shape."""
    torch, capi, pl = dev
    a, e, prm = scene["a"], scene["e"], scene["prm"]
    cloud, _ = scene["clouds"][(100, True)]
    nan = np.eye(4)
    nan[1, 2] = np.nan
    huge = np.eye(4)
    huge[0, 3] = 1e300
    other = pl.KinectFusion(dict(prm, thres_range=prm["thres_range"] + 1))
    assert other.tranc_dist() != a.tranc_dist()
    g, s = a.register_points_global, a.score_point_transforms
    calls = [lambda: a.register_map_points_global(other, cloud), lambda: a.register_map_points_global(a, cloud), lambda: g(cloud, candidates=0), lambda: g(cloud, keep=0),
             lambda: g(cloud, keep=33), lambda: g(cloud, rounds=-1), lambda: g(cloud, stride=0), lambda: g(cloud, box_t=-0.1), lambda: g(cloud, box_t=float("nan")),
             lambda: g(cloud, refine_t=-1.0), lambda: g(cloud, refine_r=float("inf")), lambda: g(cloud, refine_r=-0.1), lambda: g(cloud, iterations=-1),
             lambda: g(cloud, damping=-1.0), lambda: g(cloud, min_weight=0), lambda: g(cloud, max_residual=0.0), lambda: g(cloud, max_residual=float("nan")),
             lambda: g(cloud, Ts=nan), lambda: g(cloud, Ts=huge), lambda: g(np.zeros((0, 3))), lambda: g(np.zeros((4, 2))), lambda: g(torch.zeros(5, 3)),
             lambda: a.score_map_point_transforms(other, cloud, np.eye(4)), lambda: a.score_map_point_transforms(a, cloud, np.eye(4)), lambda: s(cloud, nan),
             lambda: s(cloud, huge), lambda: s(cloud, np.zeros((0, 4, 4))), lambda: s(cloud, np.eye(4), stride=0), lambda: s(cloud, np.eye(4), min_weight=0),
             lambda: s(cloud, np.eye(4), max_residual=float("nan")), lambda: s(np.zeros((0, 3)), np.eye(4))]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} was accepted")
    o = pl.RegisterSearchOpts()
    pl._lib.xs_kf_register_search_defaults(a.h, C.byref(o))
    assert (o.struct_bytes, o.candidates, o.keep, o.rounds, o.stride, o.iterations, o.min_weight, o.user_n) == (80, 2048, 8, 2, 4, 10, 1, 0)
    assert abs(o.box_t - a.tranc_dist()) < 1e-12 and o.box_t == o.refine_t and (o.refine_r, o.damping, o.max_residual) == (0.25, 1e-3, 0.9) and not o.user_T16xN
    out, report = np.full(16, -7.0), np.zeros(12)
    f64p = C.POINTER(C.c_double)
    call = lambda n, opts: pl._lib.xs_kf_register_points_global(a.h, n, cloud.ctypes.data, 0, C.byref(opts), out.ctypes.data_as(f64p), report.ctypes.data_as(f64p))
    # more than 2^24 scored points is refused before the cloud is read (the pointer holds far fewer): at stride 4 that is n > 2^26
    assert call((1 << 26) + 1, o) == -1 and (out == -7.0).all()
    o.stride = 1
    assert call((1 << 24) + 1, o) == -1 and (out == -7.0).all()
    o.stride = 4
    o.struct_bytes = 72
    assert call(len(cloud), o) == -1 and (out == -7.0).all()
    other.close()
    assert same_volume(a.volume(), scene["va"]) and state_of(a) == scene["states"]["a"]


def test_shard_mode_refuses(dev, scene, tmp_path):
    """Two ranks as threads on one GPU: every entry raises XsError (-2) on every rank, and the pipeline tracks the next frame afterwards."""
    torch, capi, pl = dev
    sh = importlib.import_module("x-slam_amd.sharded")
    a = scene["a"]
    cloud, _ = scene["clouds"][(100, True)]
    path = str(tmp_path / "a.ckpt")
    a.save_checkpoint(path)
    frames = [torch.from_numpy(synth.s1_frame(k).view(np.int16)).cuda() for k in range(2)]
    world = 2
    prm = dict(synth.s1_params(64), icp_shard_rows=False)
    lw = sh.LocalWorld(torch, world)
    shards = [sh.ShardedKinectFusion(prm, r, world, collective=lw.collective_for(r)) for r in range(world)]
    refused, errors = [0] * world, []

    def work(r):
        try:
            assert shards[r].process_frame(frames[0]) == 1
            k = shards[r]
            for call in (lambda: k.register_points_global(cloud), lambda: k.register_map_points_global(a, cloud), lambda: k.register_checkpoint_points_global(path, cloud),
                         lambda: k.score_point_transforms(cloud, np.eye(4)), lambda: k.score_map_point_transforms(a, cloud, np.eye(4)),
                         lambda: k.score_checkpoint_point_transforms(path, cloud, np.eye(4)), lambda: k.register_and_fuse(cloud, global_search=True)):
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
    assert refused == [7] * world
    for s in shards:
        s.close()
