"""GPU: the clearance field (xs_clearance_build), the flood over it (xs_reach_flood), the point query (xs_reach_query) and the orchestrator's
calls built on them (KinectFusion.clearance_field, reachable, next_reachable_view); DESIGN.md section 4.19.  Everything is integer
arithmetic on the observation grid's states, so every comparison is for EQUALITY with the scipy model of tests/reach_cases.py (an exact
Euclidean distance transform and a connected-component labelling).  Outputs are pre-filled with garbage and carry a guard."""
import importlib
import threading

import numpy as np
import pytest

import reach_cases as rc
import view_cases as vc
from helpers import intr_of, synth

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


def grid_of(dev, value, weight, res, min_weight=1):
    """The observation grid of dense host volumes [Z, Y, X] (a uint8 device tensor, garbage where the build writes nothing)."""
    torch, capi, _ = dev
    dv = torch.from_numpy(np.ascontiguousarray(value, np.float32).reshape(-1)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(weight, np.int32).reshape(-1)).cuda()
    grid = torch.full((capi.view_grid_bytes(res),), 0xA5, dtype=torch.uint8, device="cuda")
    capi.view_grid_build(dv, dw, res[0] * 4, res, grid, min_weight=min_weight)
    torch.cuda.synchronize()
    return grid


def grid_of_states(dev, states, res):
    return grid_of(dev, *vc.volumes_of(states), res)


def field_tensor(dev, res, fill=0x5A5A):
    torch = dev[0]
    n = res[0] * res[1] * res[2]
    return torch.full((n + GUARD,), fill, dtype=torch.int32, device="cuda").to(torch.int16)   # (0x5A5A as int16 bits)


def build_field(dev, grid, res, R, unknown_blocks):
    """uint16 [Z, Y, X] on the host and the device tensor; the output is pre-filled with 0x5A5A, the workspace with 0xC3, and the guard
    behind the field is checked."""
    torch, capi, _ = dev
    X, Y, Z = res
    n = X * Y * Z
    field = field_tensor(dev, res)
    ws = torch.full((capi.clearance_workspace_bytes(res) + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    capi.clearance_build(grid, res, R, unknown_blocks, ws, field)
    torch.cuda.synchronize()
    host = field.cpu().numpy().view(np.uint16)
    assert np.all(host[n:] == 0x5A5A) and bool((ws[-GUARD:] == 0xC3).all())
    return host[:n].reshape(Z, Y, X).copy(), field


def check_field(dev, states, res, R, unknown_blocks):
    got, _ = build_field(dev, grid_of_states(dev, states, res), res, R, unknown_blocks)
    want = rc.clearance(states, R, unknown_blocks)
    assert np.array_equal(got, want), (res, R, unknown_blocks, np.argwhere(got != want)[:5], got[got != want][:5], want[got != want][:5])
    return want


@pytest.mark.parametrize("res", [(20, 18, 13), (8, 8, 8), (19, 18, 13)])
def test_clearance_equals_the_model(dev, res):
    """Random per-voxel volumes (view_cases.random_volume through states_of: every state at every bit position, partial bricks on every
    axis between the three resolutions) and a sparse scene whose distances reach the cap, both unknown_blocks settings, R in {1, 2, 7, 40}
    (40 is longer than every axis); two builds give equal bytes."""
    torch, capi, _ = dev
    value, weight = vc.random_volume(res, seed=3 + res[0])
    dense = vc.states_of(value, weight)
    sparse = rc.random_states(res, seed=5 + res[0], p=(0.004, 0.99, 0.006))
    assert len(np.unique(dense)) == 3 and len(np.unique(sparse)) == 3
    grid = grid_of(dev, value, weight, res)
    for ub in (0, 1):
        for R in (1, 2, 7, 40):
            got, _ = build_field(dev, grid, res, R, ub)
            want = rc.clearance(dense, R, ub)
            assert np.array_equal(got, want), (R, ub, np.argwhere(got != want)[:5])
            want = check_field(dev, sparse, res, R, ub)
            print(res, "unknown_blocks", ub, "R", R, "sparse: distinct values", len(np.unique(want)), "max", want.max())
            assert want.max() == min(R * R, rc.clearance(sparse, 40, ub).max()) and (want.max() > 4 or R <= 2)
    a, fa = build_field(dev, grid_of_states(dev, sparse, res), res, 7, 1)
    b, fb = build_field(dev, grid_of_states(dev, sparse, res), res, 7, 1)
    assert torch.equal(fa, fb) and len(np.unique(a)) > 5


def test_clearance_long_and_short_axes(dev):
    """(300, 4, 5) with R = 255 and a single obstacle at x = 0: an axis longer than the window, two shorter than it, values up to 65 025.
    (3, 3, 3) with R = 40.  No obstacle at all with unknown_blocks = 0: R^2 everywhere; with unknown_blocks = 1 the outside decides."""
    res = (300, 4, 5)
    states = np.full((5, 4, 300), rc.FREE, np.uint8)
    states[2, 1, 0] = rc.OCCUPIED
    want = check_field(dev, states, res, 255, 0)
    assert want.max() == 65025 and want[2, 1, 255] == 65025 and want[2, 1, 254] == 254 * 254 and want[0, 3, 0] == 8 and want[2, 1, 0] == 0
    check_field(dev, states, res, 255, 1)
    check_field(dev, states, res, 100, 0)
    states[2, 1, 0] = rc.FREE
    states[4, 3, 299] = rc.UNKNOWN                                               # an obstacle only with unknown_blocks
    assert np.all(check_field(dev, states, res, 255, 0) == 65025)
    assert check_field(dev, states, res, 255, 1).max() == 4                      # (y has four voxels: two to the outside)
    small = rc.random_states((3, 3, 3), seed=2, p=(0.1, 0.8, 0.1))
    for ub in (0, 1):
        check_field(dev, small, (3, 3, 3), 40, ub)
    free = np.full((3, 3, 3), rc.FREE, np.uint8)
    assert np.all(check_field(dev, free, (3, 3, 3), 40, 0) == 1600)
    assert check_field(dev, free, (3, 3, 3), 40, 1)[1, 1, 1] == 4


# ---- the flood -----------------------------------------------------------------------------------------------------------------------------
def flood(dev, grid, field, res, r2, seeds):
    """(reached bool [Z, Y, X], passable bool [Z, Y, X], rounds, the reach buffer); the buffer is pre-filled with 0xEE and its guard checked."""
    torch, capi, _ = dev
    X, Y, Z = res
    n = X * Y * Z
    nbytes = capi.reach_bytes(res)
    reach = torch.full((nbytes + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    rounds = capi.reach_flood(grid, field, res, r2, seeds, reach)
    out = torch.full((2 * n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    capi.reach_expand(reach, res, out)
    capi.reach_expand(reach, res, out[n:], passable=True)
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.all(host[2 * n:] == 0x77) and bool((reach[nbytes:] == 0xEE).all()) and set(np.unique(host[:2 * n])) <= {0, 1}
    return host[:n].reshape(Z, Y, X).astype(bool), host[n:2 * n].reshape(Z, Y, X).astype(bool), rounds, reach


def check_flood(dev, states, res, R, ub, r2, seeds):
    grid = grid_of_states(dev, states, res)
    want_field = rc.clearance(states, R, ub)
    got_field, field = build_field(dev, grid, res, R, ub)
    assert np.array_equal(got_field, want_field)
    got, passable, rounds, reach = flood(dev, grid, field, res, r2, seeds)
    want = rc.reached(states, want_field, r2, seeds)
    assert np.array_equal(passable, rc.passable_of(states, want_field, r2))
    assert np.array_equal(got, want), (res, r2, int(got.sum()), int(want.sum()), np.argwhere(got != want)[:5])
    return want, rounds, dict(grid=grid, field=field, reach=reach, field_host=want_field)


@pytest.mark.parametrize("res", [(20, 18, 13), (19, 18, 13)])
def test_flood_equals_the_model(dev, res):
    """Random states at a free fraction where label finds several components; a serpentine corridor one voxel wide that crosses at least
    30 brick faces and doubles back through bricks it has left (more than one round); a corridor three voxels wide with a sideways step
    that r2 = 1 passes and r2 = 4 does not; seeds that are impassable, outside the volume, duplicated, and 64 at once; two floods equal."""
    torch, capi, _ = dev
    X, Y, Z = res
    from scipy import ndimage
    states = rc.random_states(res, seed=17, p=(0.3, 0.4, 0.3))
    field0 = rc.clearance(states, 2, 0)
    lab, ncomp = ndimage.label(rc.passable_of(states, field0, 1))
    sizes = np.bincount(lab.reshape(-1))[1:]
    print(res, "components", ncomp, "largest", np.sort(sizes)[-4:])
    assert ncomp >= 3
    big = np.argsort(sizes)[-3:] + 1
    in_comp = lambda c: tuple(int(v) for v in np.argwhere(lab == c)[0][::-1])
    blocked = tuple(int(v) for v in np.argwhere(states != rc.FREE)[0][::-1])
    for seeds in ([in_comp(big[2])], [in_comp(big[0]), in_comp(big[1])], [blocked], [(-1, 3, 3), (X, 2, 2), (3, Y, 1), (2, 2, Z), (2, -5, 2)],
                  [in_comp(big[2])] * 3 + [blocked, (X, 0, 0)]):
        want, rounds, _ = check_flood(dev, states, res, 2, 0, 1, seeds)
        print("  seeds", seeds[:2], "reached", int(want.sum()), "rounds", rounds)
        assert rounds >= 1
    assert not check_flood(dev, states, res, 2, 0, 1, [blocked])[0].any()
    rng = np.random.default_rng(8)
    many = np.stack([rng.integers(-1, X + 1, 64), rng.integers(-1, Y + 1, 64), rng.integers(-1, Z + 1, 64)], axis=1)
    want, _, keep = check_flood(dev, states, res, 2, 0, 1, many)
    assert want.sum() > sizes.max() and not want.all()
    again = flood(dev, keep["grid"], keep["field"], res, 1, many)[3]
    words = 16 * -(-X // 4) * -(-Y // 4) * -(-Z // 4)                           # (behind them the flood's control words: they follow the rounds)
    assert torch.equal(again[:words], keep["reach"][:words])
    roomy = rc.random_states(res, seed=19, p=(0.01, 0.97, 0.02))                 # unknown voxels and the outside block; wider bodies
    for r2 in (2, 3, 5):
        want, rounds, _ = check_flood(dev, roomy, res, 3, 1, r2, many)
        print("  roomy r2", r2, "reached", int(want.sum()), "rounds", rounds)
        assert want.any() and not want.all()
    # the serpentine
    s, path = rc.serpentine(res)
    crossed = rc.brick_faces_crossed(path)
    assert crossed >= 30 and len({tuple(c >> 2 for c in v) for v in path[:X - 2]} & {tuple(c >> 2 for c in v) for v in path[X - 1:2 * X - 3]}) >= 4
    want, rounds, _ = check_flood(dev, s, res, 1, 0, 1, [path[0]])
    print("  serpentine: voxels", len(path), "brick faces crossed", crossed, "rounds", rounds)
    assert want.sum() == len(path) and all(want[z, y, x] for x, y, z in path) and rounds > 1
    want, rounds2, _ = check_flood(dev, s, res, 1, 0, 1, [path[-1], path[len(path) // 2]])
    assert want.sum() == len(path) and rounds2 > 1
    # the corridor with a step
    s, start, goal = rc.jogged_corridor(res)
    w1, _, _ = check_flood(dev, s, res, 2, 0, 1, [start])
    w4, _, _ = check_flood(dev, s, res, 2, 0, 4, [start])
    assert w1[goal[2], goal[1], goal[0]] and w4[start[2], start[1], start[0]] and not w4[goal[2], goal[1], goal[0]] and w4.sum() > 3


@pytest.fixture(scope="module")
def scene(dev):
    """The query test's inputs, computed once: random states on (19, 18, 13), the field at R = 3 with unknown_blocks, a flood at r2 = 1."""
    res = (19, 18, 13)
    states = rc.random_states(res, seed=23, p=(0.2, 0.55, 0.25))
    seeds = [(9, 9, 6), (3, 3, 3), (15, 12, 9), (10, 4, 2)]
    want, rounds, keep = check_flood(dev, states, res, 3, 1, 1, seeds)
    assert want.any() and not want.all()
    return dict(res=res, states=states, reached=want, passable=rc.passable_of(states, keep["field_host"], 1), **keep)


def run_query(dev, scene, points, voxel_size, snap, over_passable=False):
    torch, capi, _ = dev
    n = len(points)
    dp = torch.from_numpy(np.ascontiguousarray(points, np.float32).reshape(-1)).cuda()
    flags = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    clear2 = torch.full((n + GUARD,), 0x5A5A, dtype=torch.int32, device="cuda").to(torch.int16)
    voxel = torch.full((3 * n + GUARD,), -77, dtype=torch.int32, device="cuda")
    capi.reach_query(n, dp, scene["res"], voxel_size, scene["reach"], scene["field"], flags, clear2, snap=snap, over_passable=over_passable, voxel=voxel)
    torch.cuda.synchronize()
    f, c, v = flags.cpu().numpy(), clear2.cpu().numpy().view(np.uint16), voxel.cpu().numpy()
    assert np.all(f[n:] == 0x77) and np.all(c[n:] == 0x5A5A) and np.all(v[3 * n:] == -77)
    return f[:n], c[:n], v[:3 * n].reshape(n, 3)


def test_query_equals_the_model(dev, scene):
    """200 points: inside, outside, exactly on voxel faces (integer multiples of a binary voxel size and of 0.05), 20 m away and a NaN;
    snap 0 and 3 over the reached words and over the passable ones; among the snapped answers there are ties, which go to the lowest linear
    index."""
    X, Y, Z = scene["res"]
    rng = np.random.default_rng(31)
    for vs in (np.float32(0.0625), np.float32(0.05)):
        ext = np.array([X, Y, Z], np.float32) * vs
        inside = (rng.uniform(0, 1, size=(120, 3)) * ext).astype(np.float32)
        around = (rng.uniform(-0.2, 1.2, size=(40, 3)) * ext).astype(np.float32)
        faces = (rng.integers(0, [X + 1, Y + 1, Z + 1], size=(36, 3)).astype(np.float32) * vs).astype(np.float32)
        far = np.array([[20.0, 0.4, 0.3], [0.4, -20.0, 0.3], [0.4, 0.3, 20.0], [np.nan, 0.4, 0.3]], np.float32)
        pts = np.concatenate([inside, around, faces, far])
        assert len(pts) == 200
        ties = 0
        for over, mask in ((False, scene["reached"]), (True, scene["passable"])):
            for snap in (0, 3):
                f, c, v = run_query(dev, scene, pts, vs, snap, over_passable=over)
                wf, wc, wv = rc.query(pts, vs, mask, scene["field_host"], snap)
                assert np.array_equal(f, wf) and np.array_equal(c, wc) and np.array_equal(v, wv), (vs, over, snap, np.flatnonzero((f != wf) | (c != wc))[:5])
                if snap:
                    f0 = rc.query(pts, vs, mask, scene["field_host"], 0)[0]
                    moved = np.flatnonzero((wf == 1) & (f0 == 0))
                    for i in moved:
                        s = rc.voxel_of(pts[i], vs)[0].astype(int)
                        d2 = int(((wv[i] - s) ** 2).sum())
                        zz, yy, xx = np.nonzero(mask)
                        near = (np.abs(xx - s[0]) <= snap) & (np.abs(yy - s[1]) <= snap) & (np.abs(zz - s[2]) <= snap)
                        ties += int((((xx - s[0]) ** 2 + (yy - s[1]) ** 2 + (zz - s[2]) ** 2)[near] == d2).sum() > 1)
                    print("voxel", vs, "passable" if over else "reached", "snap", snap, "answers 1:", int(wf.sum()), "snapped:", len(moved))
                    assert len(moved) >= 5
        assert ties >= 3
        assert not wf[-4:].any() and not wc[-4:].any()


def test_argument_checks(dev, scene):
    """Every refused call returns hipErrorInvalidValue (XsError) and leaves its outputs untouched."""
    torch, capi, _ = dev
    res = scene["res"]
    n = res[0] * res[1] * res[2]
    grid, good_field, good_reach = scene["grid"], scene["field"], scene["reach"]
    field = field_tensor(dev, res)
    ws = torch.full((capi.clearance_workspace_bytes(res),), 0xC3, dtype=torch.uint8, device="cuda")
    for R, ub, r, g, w, f in ((0, 0, res, grid, ws, field), (256, 0, res, grid, ws, field), (-3, 1, res, grid, ws, field), (4, 2, res, grid, ws, field),
                              (4, 0, (19, 0, 13), grid, ws, field), (4, 0, (19, 18, -1), grid, ws, field), (4, 0, res, None, ws, field),
                              (4, 0, res, grid, None, field), (4, 0, res, grid, ws, None)):
        with pytest.raises(capi.XsError):
            capi.clearance_build(g, r, R, ub, w, f)
    torch.cuda.synchronize()
    assert bool((field.view(torch.uint8) == 0x5A).all()) and bool((ws == 0xC3).all())
    reach = torch.full((capi.reach_bytes(res),), 0xEE, dtype=torch.uint8, device="cuda")
    one = [(3, 3, 3)]
    for r2, seeds, r, g, f, out in ((0, one, res, grid, good_field, reach), (-4, one, res, grid, good_field, reach), (1, np.zeros((0, 3), np.int32), res, grid, good_field, reach),
                                    (1, np.zeros((65, 3), np.int32), res, grid, good_field, reach), (1, one, (0, 18, 13), grid, good_field, reach),
                                    (1, one, res, None, good_field, reach), (1, one, res, grid, None, reach), (1, one, res, grid, good_field, None)):
        with pytest.raises(capi.XsError):
            capi.reach_flood(g, f, r, r2, seeds, out)
    with pytest.raises(capi.XsError):
        capi.reach_passable(grid, good_field, res, 0, reach)
    with pytest.raises(capi.XsError):
        capi.reach_expand(None, res, reach)
    torch.cuda.synchronize()
    assert bool((reach == 0xEE).all())
    pts = torch.zeros(3 * 8, dtype=torch.float32, device="cuda")
    flags = torch.full((8,), 0x77, dtype=torch.uint8, device="cuda")
    clear2 = torch.full((8,), 0x5A5A, dtype=torch.int32, device="cuda").to(torch.int16)
    for kw in (dict(n=0), dict(snap=-1), dict(snap=17), dict(voxel_size=0.0), dict(voxel_size=float("nan")), dict(res=(19, 18, 0)), dict(points=None),
               dict(reach=None), dict(field=None), dict(reachable=None), dict(clear2=None)):
        a = dict(n=8, points=pts, res=res, voxel_size=0.05, reach=good_reach, field=good_field, reachable=flags, clear2=clear2, snap=2)
        a.update(kw)
        with pytest.raises(capi.XsError):
            capi.reach_query(**a)
    torch.cuda.synchronize()
    assert bool((flags == 0x77).all()) and bool((clear2.view(torch.uint8) == 0x5A).all())
    capi.reach_query(8, pts, res, 0.05, good_reach, good_field, flags, clear2, snap=16)   # the edge of the valid range does launch
    torch.cuda.synchronize()
    assert bool((flags <= 1).all())


# ---- orchestrator level ----------------------------------------------------------------------------------------------------------------
# The candidate box and the body: 64 pose_candidates within +-0.3 m and +-0.3 rad of the last tracked pose of scene S3 at 64^3 (the section
# 4.18 test's setting; a voxel is 0.12 m), a body of 0.1 m (r2 = 1, R = 1).  Four frames carve a narrow cone of some 2 900 FREE voxels in
# front of the camera out of 262 144; the camera's own voxel is UNKNOWN and the start snaps one voxel forward.  Candidates moved forward into
# the cone are reachable, those moved sideways or backwards sit in never-observed space: the model puts 3 of the 64 in the first class, and
# the test asserts that both classes occur.
ORCH_BOX_T, ORCH_RADIUS = 0.3, 0.1


def model_of_kf(kf, prm, cands, radius_m, snap, unknown_blocks, start=None, min_weight=1):
    n = kf.res[0]
    v, w, _ = kf.volume()
    states = vc.states_of(v.reshape(n, n, n), w.reshape(n, n, n), min_weight)
    vs = prm["tsdf_voxel_size"]
    r2, R = rc.radius_of(radius_m, vs)
    field = rc.clearance(states, R, unknown_blocks)
    passable = rc.passable_of(states, field, r2)
    s = kf.camera2volume() if start is None else start
    found, _, seed = rc.query(np.asarray(s, np.float32)[:3, 3, 0][None], vs, passable, field, snap)
    reached = rc.reached(states, field, r2, seed if found[0] else [(-1, -1, -1)])
    flags, clear2, _ = rc.query(cands[:, :3, 3, 0], vs, reached, field, 0)
    return dict(states=states, field=field, r2=r2, R=R, seed=seed[0], found=bool(found[0]), reached=reached, flags=flags.astype(bool), clear2=clear2)


def test_orchestrator_follows_the_volume(dev):
    """Scene S3 fused for four frames at 64^3 through KinectFusion; 64 pose_candidates around the last pose.  clearance_field and reachable
    equal the model on the downloaded volume(); the model puts candidates in both classes; next_reachable_view equals the model's pick and
    is a reachable candidate; next_best_view on the same inputs is what it was; after one more frame the answers are recomputed and again
    equal the model."""
    torch, capi, pl = dev
    n = 64
    prm = synth.s1_params(n)
    kf = pl.KinectFusion(prm)
    dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(5)]
    for k in range(4):
        assert kf.process_frame(dfr[k]) == 1
    cands = pl.pose_candidates(kf.camera2volume(), ORCH_BOX_T, 0.3, 64)
    before_best, before_counts = kf.next_best_view(cands)

    def check(tag):
        m = model_of_kf(kf, prm, cands, ORCH_RADIUS, 4, 1)
        for R, ub in ((m["R"], 1), (5, 0)):
            got = kf.clearance_field(R, unknown_blocks=bool(ub))
            want = m["field"] if ub else rc.clearance(m["states"], R, 0)
            assert got.shape == (n, n, n) and got.dtype == np.uint16 and np.array_equal(got, want), (tag, R, ub)
        flags, clear2 = kf.reachable(cands, ORCH_RADIUS)
        print(tag, "r2", m["r2"], "R", m["R"], "seed", m["seed"], "reached voxels", int(m["reached"].sum()), "reachable candidates", int(m["flags"].sum()),
              "of 64")
        assert m["found"] and 0 < m["flags"].sum() < 64
        assert flags.dtype == bool and np.array_equal(flags, m["flags"]) and np.array_equal(clear2, m["clear2"])
        again = kf.reachable(cands, ORCH_RADIUS)                                 # (from the cache)
        assert np.array_equal(again[0], flags) and np.array_equal(again[1], clear2)
        return m, flags

    m, flags = check("after four frames:")
    # another start, another body, no unknown_blocks, no snap: each recomputes and equals the model
    for kw in (dict(start=cands[int(np.flatnonzero(m["flags"])[0])]), dict(radius_m=0.2), dict(radius_m=0.2, unknown_blocks=False), dict(unknown_blocks=False), dict(snap_vox=0), dict(min_weight=2)):
        a = dict(radius_m=ORCH_RADIUS, start=None, snap_vox=4, unknown_blocks=True, min_weight=1)
        a.update(kw)
        mm = model_of_kf(kf, prm, cands, a["radius_m"], a["snap_vox"], int(a["unknown_blocks"]), start=a["start"], min_weight=a["min_weight"])
        f, c = kf.reachable(cands, a.pop("radius_m"), **a)
        print("  ", list(kw), "reachable", int(mm["flags"].sum()), "seed found", mm["found"])
        assert np.array_equal(f, mm["flags"]) and np.array_equal(c, mm["clear2"]), kw
    best, counts, rflags = kf.next_reachable_view(cands, ORCH_RADIUS)
    want_best = rc.next_reachable_view(before_counts, m["flags"], 80 * 60 // 4)
    print("next reachable view", best, "next best view", before_best)
    assert np.array_equal(counts, before_counts) and np.array_equal(rflags, m["flags"]) and best == want_best
    assert best < 0 or rflags[best]
    lo = kf.next_reachable_view(cands, ORCH_RADIUS, min_hits=0)
    assert lo[0] == rc.next_reachable_view(before_counts, m["flags"], 0) and lo[0] >= 0 and rflags[lo[0]]
    assert kf.next_reachable_view(cands, ORCH_RADIUS, min_hits=10 ** 9)[0] == -1
    again_best, again_counts = kf.next_best_view(cands)                          # what it was
    assert again_best == before_best and np.array_equal(again_counts, before_counts)
    for bad in (dict(radius_m=40.0), dict(radius_m=-1.0), dict(radius_m=ORCH_RADIUS, snap_vox=17), dict(radius_m=float("nan"))):
        with pytest.raises(ValueError):
            kf.reachable(cands, **bad)
    with pytest.raises(ValueError):
        kf.clearance_field(256)
    with pytest.raises(ValueError):
        kf.next_reachable_view(cands, 40.0)                                      # 333 voxels: R would exceed 255
    assert kf.process_frame(dfr[4]) == 1
    m2, flags2 = check("after one more frame:")
    assert (m2["field"] != m["field"]).any()
    kf.close()


def test_shard_mode_refuses(dev):
    """Two ranks as threads on one GPU: clearance_field, reachable and next_reachable_view raise XsError on every rank and do nothing, and
    the pipeline tracks the next frame afterwards."""
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
            for call in (lambda: shards[r].clearance_field(4), lambda: shards[r].reachable(cands, 0.06), lambda: shards[r].next_reachable_view(cands, 0.06)):
                try:
                    call()
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
    assert refused == [3] * world
    assert np.array_equal(shards[0].world2camera(), shards[1].world2camera())
    for s in shards:
        s.close()
