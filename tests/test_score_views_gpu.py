"""GPU: the two-bit observation grid (xs_view_grid_build / _expand), the scoring of many candidate views in one launch (xs_score_views,
k_score_views) and the next-best-view calls built on them (KinectFusion.score_views, next_best_view); DESIGN.md section 4.18.  Counts are
compared for EQUALITY with the float32 numpy model of the contract (tests/view_cases.py): the kernel does the same IEEE operations in the
same order and adds integers, so there is no flip budget.  A count that differs means the kernel broke the order of operations."""
import importlib
import threading

import numpy as np
import pytest

import view_cases as vc
from helpers import intr_of, synth

pytestmark = pytest.mark.gpu
GARBAGE = 0xDEADBEEF
GARBAGE_I32 = GARBAGE - (1 << 32)   # the same bits in the int32 tensors the counts are kept in (torch has few uint32 operations)


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


def build_grid(dev, value, weight, res, min_weight=1, pitch=None, offset=0):
    """The grid of dense host volumes [Z, Y, X] as a uint8 device tensor.  pitch: floats per stored row (None: X); offset: floats the
    volumes' base pointers are moved off their allocation (alignment)."""
    torch, capi, _ = dev
    X, Y, Z = res
    pitch = X if pitch is None else pitch
    hv, hw = np.full((Z * Y, pitch), 7.0, np.float32), np.full((Z * Y, pitch), 9, np.int32)   # (the padding: known and free, were it read)
    hv[:, :X], hw[:, :X] = np.asarray(value, np.float32).reshape(Z * Y, X), np.asarray(weight, np.int32).reshape(Z * Y, X)
    dv, dw = torch.zeros(Z * Y * pitch + offset, dtype=torch.float32, device="cuda"), torch.zeros(Z * Y * pitch + offset, dtype=torch.int32, device="cuda")
    dv[offset:] = torch.from_numpy(hv.reshape(-1)).cuda()
    dw[offset:] = torch.from_numpy(hw.reshape(-1)).cuda()
    grid = torch.full((capi.view_grid_bytes(res),), 0xA5, dtype=torch.uint8, device="cuda")
    capi.view_grid_build(dv.data_ptr() + 4 * offset, dw.data_ptr() + 4 * offset, pitch * 4, res, grid, min_weight=min_weight)
    torch.cuda.synchronize()
    return grid


def expand(dev, grid, res):
    torch, capi, _ = dev
    X, Y, Z = res
    states = torch.full((X * Y * Z,), 0xEE, dtype=torch.uint8, device="cuda")
    capi.view_grid_expand(grid, res, states)
    torch.cuda.synchronize()
    return states.cpu().numpy().reshape(Z, Y, X)


def score(dev, grid, res, voxel_size, R, t, opts=None, intr=vc.INTR, rows=vc.ROWS, cols=vc.COLS):
    """One launch of xs_score_views for the poses R [P, 3, 3], t [P, 3]: uint32 [P, 4]; `out` is pre-filled with garbage and has a guard."""
    torch, capi, _ = dev
    P = len(R)
    out = torch.full((4 * P + 4,), GARBAGE_I32, dtype=torch.int32, device="cuda")
    capi.score_views(R, t, intr, rows, cols, res, float(voxel_size), grid, out, opts=opts)
    torch.cuda.synchronize()
    host = out.cpu().numpy().view(np.uint32)
    assert np.all(host[4 * P:] == GARBAGE)
    return host[:4 * P].reshape(P, 4)


@pytest.mark.parametrize("res", [(20, 18, 13), (8, 8, 8), (19, 18, 13)])
def test_grid_equals_the_numpy_states(dev, res):
    """xs_view_grid_expand of the built grid against the rule in numpy, per-voxel random volumes (weights from {0, 1, 2, 5}, values from
    {-0.5, 0, 1, -0.0f, -1e-30}: every bit position of a brick word takes every state), min_weight 1 and 3 (and 0, which means 1).
    (20, 18, 13): partial bricks in y and z; (8, 8, 8): aligned; (19, 18, 13): partial in x too — those bricks take the per-voxel path.
    Pitched volumes: a 16-byte multiple pitch (the 16-byte loads) and one that is not (the exact path), and base pointers 4 bytes off a
    16-byte boundary.  Two builds give the same bytes."""
    torch, capi, _ = dev
    X, Y, Z = res
    value, weight = vc.random_volume(res, seed=7 + X)
    nbricks = -(-X // 4) * -(-Y // 4) * -(-Z // 4)
    for mw in (1, 3, 0):
        want = vc.states_of(value, weight, mw)
        assert len(np.unique(want)) == 3
        grid = build_grid(dev, value, weight, res, mw)
        got = expand(dev, grid, res)
        assert np.array_equal(got, want), (mw, np.argwhere(got != want)[:5])
        again = build_grid(dev, value, weight, res, mw)
        assert torch.equal(grid[:16 * nbricks], again[:16 * nbricks])
        for pitch, offset in ((X + 4 - X % 4 + 4, 0), (X + 3 if (X + 3) % 4 else X + 5, 0), (X, 1), (X + 4 - X % 4, 3)):
            g2 = build_grid(dev, value, weight, res, mw, pitch=pitch, offset=offset)
            assert torch.equal(g2[:16 * nbricks], grid[:16 * nbricks]), (mw, pitch, offset)
    with pytest.raises(capi.XsError):
        capi.view_grid_build(grid, grid, X * 4 - 4, res, grid)                  # a pitch shorter than a row
    with pytest.raises(capi.XsError):
        capi.view_grid_build(grid, grid, X * 4, (X, 0, Z), grid)


@pytest.fixture(scope="module")
def case(dev):
    """The kernel-versus-model inputs, computed once and left unchanged: two volumes of (20, 18, 13) voxels of 0.05 m — `sparse` (45 %
    unknown, 50 % free, 5 % occupied: long rays with frontier crossings) and `dense` (the per-voxel random volume of the grid test: rays
    end within a few voxels) — and 69 poses."""
    rng = np.random.default_rng(21)
    X, Y, Z = vc.CASE_RES
    sparse = rng.choice(np.array([0, 1, 2], np.uint8), size=(Z, Y, X), p=[0.45, 0.5, 0.05])
    dense = vc.states_of(*vc.random_volume(vc.CASE_RES, seed=5))
    R, t, names = vc.case_poses(n_random=64)
    grids = {"sparse": build_grid(dev, *vc.volumes_of(sparse), vc.CASE_RES), "dense": build_grid(dev, *vc.random_volume(vc.CASE_RES, seed=5), vc.CASE_RES)}
    return dict(states={"sparse": sparse, "dense": dense}, grids=grids, R=R, t=t, names=names)


def case_opts(capi, rays):
    return capi.view_opts(rays, vc.CASE_NEAR, vc.CASE_FAR, vc.CASE_STEP)


@pytest.mark.parametrize("rays", [(8, 8), (9, 7), (80, 60)])
@pytest.mark.parametrize("which", ["sparse", "dense"])
def test_kernel_equals_the_model(dev, case, which, rays):
    """Every pose's four counts against the model, 36 samples per ray: one wave (8 x 8), partial tiles (9 x 7) and the default lattice.
    The poses: inside the volume, outside looking in, looking away and 20 m off (all zeros), identity with t on exact multiples of the
    voxel size (samples on voxel faces) and random rigid poses."""
    torch, capi, _ = dev
    assert len(vc.sample_depths(vc.CASE_NEAR, vc.CASE_FAR, vc.CASE_STEP)) == 36
    n = 29                                                                       # the five named poses and 24 random ones
    R, t = case["R"][:n], case["t"][:n]
    got = score(dev, case["grids"][which], vc.CASE_RES, vc.CASE_VOXEL, R, t, case_opts(capi, rays))
    want = vc.model_poses(case["states"][which], R, t, vc.INTR, vc.ROWS, vc.COLS, vc.CASE_VOXEL, rays=rays, t_near=vc.CASE_NEAR, t_far=vc.CASE_FAR,
                          step=vc.CASE_STEP)
    print(which, rays, "totals", want.sum(axis=0), "poses with a count", int(want.any(axis=1).sum()))
    for p in np.flatnonzero((got != want).any(axis=1)):
        print("  differs:", case["names"][p], got[p], want[p])
    assert np.array_equal(got, want)
    names = case["names"]
    assert not want[names.index("looking_away")].any() and not want[names.index("far_off")].any()
    assert want[names.index("inside")].any() and want[names.index("outside_looking_in")].any() and want[names.index("on_voxel_faces")].any()
    assert np.all(want.sum(axis=0) > 0) and int(want.any(axis=1).sum()) >= 15    # unknown, free, hits and frontier crossings all occur


def test_tiles_and_independence(dev, case):
    """P = 1, 63, 64, 65 and 69: pose p's four numbers are the same in every launch that holds it, in a launch of that pose alone, in other
    slots among other poses, and on a second launch."""
    torch, capi, _ = dev
    opts = case_opts(capi, (80, 60))
    run = lambda sel: score(dev, case["grids"]["sparse"], vc.CASE_RES, vc.CASE_VOXEL, case["R"][sel], case["t"][sel], opts)
    full = run(np.arange(69))
    assert len({full[p].tobytes() for p in range(69)}) > 30
    for P in (1, 63, 64, 65):
        assert np.array_equal(run(np.arange(P)), full[:P]), P
    assert run(np.arange(69)).tobytes() == full.tobytes()
    for p in (0, 4, 5, 62, 63, 64, 68):
        assert np.array_equal(run(np.array([p]))[0], full[p]), p
    mixed = np.array([68, 5, 5, 64, 0, 63] + list(range(10, 40)))
    got = run(mixed)
    for slot, p in enumerate(mixed):
        assert np.array_equal(got[slot], full[p]), (slot, p)


def test_known_answers(dev):
    """The table of DESIGN.md section 4.18 from volumes_of(states) uploaded dense, with the library's defaults (opts NULL: 80 x 60 rays,
    0.2 .. 5.0, a voxel per step = 103 samples) and again with the same options spelled out."""
    torch, capi, _ = dev
    res = (vc.KNOWN_N,) * 3
    states = vc.known_states()
    grid = build_grid(dev, *vc.volumes_of(states), res)
    assert np.array_equal(expand(dev, grid, res), states)
    R, t = vc.known_poses()
    got = score(dev, grid, res, vc.KNOWN_VOXEL, R, t, None)
    print(got)
    assert np.array_equal(got, vc.KNOWN_COUNTS)
    assert np.array_equal(score(dev, grid, res, vc.KNOWN_VOXEL, R, t, capi.view_opts((80, 60), 0.2, 5.0, vc.KNOWN_VOXEL)), vc.KNOWN_COUNTS)
    assert vc.next_best_view(got, vc.KNOWN_MIN_HITS) == vc.KNOWN_BEST


def test_argument_checks(dev, case):
    """Each invalid call returns hipErrorInvalidValue (XsError), launches nothing and leaves `out` untouched."""
    torch, capi, _ = dev
    grid = case["grids"]["sparse"]
    out = torch.full((4 * 4100,), GARBAGE_I32, dtype=torch.int32, device="cuda")
    R1, t1 = case["R"][:1], case["t"][:1]
    many = np.arange(4097) % 69

    def refused(R, t, opts, rows=vc.ROWS, cols=vc.COLS, voxel=vc.CASE_VOXEL, res=vc.CASE_RES):
        with pytest.raises(capi.XsError):
            capi.score_views(R, t, vc.INTR, rows, cols, res, float(voxel), grid, out, opts=opts)

    ok = case_opts(capi, (8, 8))
    refused(case["R"][:0], case["t"][:0], ok)                                   # poses = 0
    refused(case["R"][many], case["t"][many], ok)                               # poses = 4097
    for rays in ((0, 8), (8, 0), (-1, 8), (8, -8), (vc.COLS + 1, 8), (8, vc.ROWS + 1)):
        refused(R1, t1, case_opts(capi, rays))                                  # a lattice dimension below 1 or above cols / rows
    refused(R1, t1, capi.view_opts((8, 8), vc.CASE_NEAR, vc.CASE_FAR, -0.05))   # step <= 0
    refused(R1, t1, capi.view_opts((8, 8), vc.CASE_NEAR, vc.CASE_FAR, float("nan")))
    refused(R1, t1, capi.view_opts((8, 8), vc.CASE_NEAR, vc.CASE_FAR, None), voxel=0.0)   # the default step is the voxel size: not positive
    refused(R1, t1, capi.view_opts((8, 8), 0.5, 0.5, 0.05))                     # t_far <= t_near
    refused(R1, t1, capi.view_opts((8, 8), 0.5, 0.25, 0.05))
    refused(R1, t1, capi.view_opts((8, 8), 0.2, 5.0, 0.001))                    # 4800 samples per ray
    refused(R1, t1, capi.view_opts((8, 8), 0.0, 4097.0, 1.0))                   # 4097 samples
    refused(R1, t1, capi.view_opts((2048, 2048), 0.5, 1024.5, 1.0), rows=2048, cols=2048)   # 2^22 rays x 1024 samples = 2^32
    bad = case_opts(capi, (8, 8)); bad.struct_bytes = 20
    refused(R1, t1, bad)
    refused(R1, t1, ok, res=(20, 0, 13))
    torch.cuda.synchronize()
    assert bool((out == GARBAGE_I32).all())
    # the edges of the valid range do launch: 4096 samples, and a lattice as large as the image
    capi.score_views(R1, t1, vc.INTR, vc.ROWS, vc.COLS, vc.CASE_RES, float(vc.CASE_VOXEL), grid, out, opts=capi.view_opts((8, 8), 0.0, 4096.0, 1.0))
    capi.score_views(R1, t1, vc.INTR, 8, 8, vc.CASE_RES, float(vc.CASE_VOXEL), grid, out[4:], opts=case_opts(capi, (8, 8)))
    torch.cuda.synchronize()
    assert bool((out[:8] != GARBAGE_I32).all()) and bool((out[8:] == GARBAGE_I32).all())


def test_resolution_beyond_a_launch_extent(dev):
    """(4, 65536, 4): Y does not fit a launch's grid dimension.  The calls that run over bricks take it (the grid has a size and builds: an
    all-FREE volume gives 0x55 in every byte of the 65536 brick words); the calls that run over voxels or tiles refuse it: xs_view_grid_expand
    with hipErrorInvalidValue (1) before any launch, and the clearance, reach, travel and frontier buffers have no size."""
    torch, capi, _ = dev
    res = (4, 65536, 4)
    X, Y, Z = res
    nbricks = 1 * (Y // 4) * 1
    assert capi.view_grid_bytes(res) >= 16 * nbricks
    value = torch.ones(X * Y * Z, dtype=torch.float32, device="cuda")
    weight = torch.ones(X * Y * Z, dtype=torch.int32, device="cuda")
    grid = torch.full((capi.view_grid_bytes(res),), 0xA5, dtype=torch.uint8, device="cuda")
    capi.view_grid_build(value, weight, X * 4, res, grid)
    torch.cuda.synchronize()
    assert bool((grid[:16 * nbricks] == 0x55).all())
    states = torch.full((X * Y * Z,), 0xEE, dtype=torch.uint8, device="cuda")
    with pytest.raises(capi.XsError, match=r"hip error 1: xs_view_grid_expand: bad resolution"):
        capi.view_grid_expand(grid, res, states)
    torch.cuda.synchronize()
    assert bool((states == 0xEE).all())
    for sized in (capi.clearance_bytes, capi.reach_bytes, capi.travel_bytes, capi.frontier_mask_bytes, capi.frontier_label_bytes):
        assert sized(res) == 0, sized.__name__


# ---- orchestrator level ----------------------------------------------------------------------------------------------------------------
def model_of_volume(kf, prm, c2vs, **kw):
    n = kf.res[0]
    v, w, _ = kf.volume()
    states = vc.states_of(v.reshape(n, n, n), w.reshape(n, n, n), kw.pop("min_weight", 1))
    return vc.model_poses(states, c2vs[:, :3, :3, 0], c2vs[:, :3, 3, 0], intr_of(prm), synth.HEIGHT, synth.WIDTH, prm["tsdf_voxel_size"], **kw), states


def test_orchestrator_follows_the_volume(dev):
    """Scene S3 fused for four frames at 64^3 through KinectFusion; 64 pose_candidates around the last pose.  score_views equals the model
    on the downloaded volume() (default options, and a 9 x 7 lattice with other depths at min_weight 2); next_best_view equals the model's
    pick, and the winner sees more unknown samples than the last tracked pose; after one more frame the scores follow the new volume; 4101
    poses go through the chunking."""
    torch, capi, pl = dev
    n = 64
    prm = synth.s1_params(n)
    kf = pl.KinectFusion(prm)
    dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(5)]
    for k in range(4):
        assert kf.process_frame(dfr[k]) == 1
    last = kf.camera2volume()
    cands = pl.pose_candidates(last, 0.3, 0.3, 64)
    got = kf.score_views(cands)
    want, states = model_of_volume(kf, prm, cands)
    print("states unknown / free / occupied:", np.bincount(states.reshape(-1), minlength=3), " totals", want.sum(axis=0))
    assert got.shape == (64, 4) and got.dtype == np.uint32 and np.array_equal(got, want) and np.all(want.sum(axis=0) > 0)
    kw = dict(rays=(9, 7), t_near=0.5, t_far=3.0, step=0.1)
    got2 = kf.score_views(cands, min_weight=2, **kw)
    want2, _ = model_of_volume(kf, prm, cands, min_weight=2, **kw)
    assert np.array_equal(got2, want2) and want2.any() and np.array_equal(kf.score_views(cands), got)   # (the grid went to gate 2 and back)
    best, counts = kf.next_best_view(cands)
    here = kf.score_views(last[None])[0]
    print("next best view", best, counts[best], " the last tracked pose sees", here)
    assert np.array_equal(counts, got) and best == vc.next_best_view(want, 80 * 60 // 4) and best >= 0
    assert counts[best, 2] >= 1200 and counts[best, 0] > here[0]
    assert kf.next_best_view(cands, min_hits=10 ** 9)[0] == -1 and kf.next_best_view(cands, min_hits=0)[0] == int(np.argmax(want[:, 0]))
    with pytest.raises(ValueError):
        kf.score_views(cands, rays=(0, 5))
    with pytest.raises(ValueError):
        kf.next_best_view(cands, t_near=1.0, t_far=0.5)
    many = np.concatenate([cands] * 65)[:4096 + 5]
    big = kf.score_views(many)
    assert big.shape == (4101, 4) and np.array_equal(big[:4096].reshape(64, 64, 4), np.broadcast_to(got, (64, 64, 4))) and np.array_equal(big[4096:], got[:5])
    assert kf.process_frame(dfr[4]) == 1
    got3 = kf.score_views(cands)
    want3, _ = model_of_volume(kf, prm, cands)
    print("candidates whose counts changed after one more frame:", int((got3 != got).any(axis=1).sum()), "of 64")
    assert np.array_equal(got3, want3) and (got3 != got).any()
    kf.close()


def test_shard_mode_refuses(dev):
    """Two ranks as threads on one GPU: score_views and next_best_view raise XsError on every rank and do nothing, and the pipeline tracks
    the next frame afterwards."""
    torch, capi, pl = dev
    sh = importlib.import_module("x-slam_amd.sharded")
    world, n = 2, 64
    prm = dict(synth.s1_params(n), icp_shard_rows=False)
    dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(2)]
    lw = sh.LocalWorld(torch, world)
    shards = [sh.ShardedKinectFusion(prm, r, world, collective=lw.collective_for(r)) for r in range(world)]
    refused, errors = [0] * world, []

    def work(r):
        try:
            assert shards[r].process_frame(dfr[0]) == 1
            cands = pl.pose_candidates(shards[r].camera2volume(), 0.3, 0.3, 8)
            for call in (shards[r].score_views, shards[r].next_best_view):
                try:
                    call(cands)
                except capi.XsError:
                    refused[r] += 1
            assert shards[r].process_frame(dfr[1]) == 1
        except BaseException as e:  # noqa: BLE001
            errors.append(e)
            lw.barrier.abort()

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errors, errors
    assert refused == [2] * world
    assert np.array_equal(shards[0].world2camera(), shards[1].world2camera())
    for s in shards:
        s.close()
