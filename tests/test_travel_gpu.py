"""GPU: the travel field (xs_travel_build), the walk down it (xs_travel_path), the voxel query (xs_travel_query) and the orchestrator's calls
built on them (KinectFusion.travel, path_to, next_view_by_travel); DESIGN.md section 4.20.  Everything is integer arithmetic, so every
comparison is for EQUALITY with the dijkstra model of tests/travel_cases.py.  Outputs are pre-filled with garbage and carry a guard."""
import importlib
import threading

import numpy as np
import pytest

import reach_cases as rc
import travel_cases as tc
import view_cases as vc
from helpers import synth

pytestmark = pytest.mark.gpu
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


def u16_tensor(dev, n, fill=0x5A5A):
    torch = dev[0]
    return torch.full((n,), fill, dtype=torch.int32, device="cuda").to(torch.int16)


def flooded(dev, states, res, R, ub, r2, seeds):
    """(reach buffer, reached bool [Z, Y, X]): the observation grid of the states, the clearance field and the flood on the GPU; the reached
    set is held to reach_cases' model before anything is built over it."""
    torch, capi, _ = dev
    X, Y, Z = res
    n = X * Y * Z
    value, weight = vc.volumes_of(states)
    dv = torch.from_numpy(np.ascontiguousarray(value, np.float32).reshape(-1)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(weight, np.int32).reshape(-1)).cuda()
    grid = torch.full((capi.view_grid_bytes(res),), 0xA5, dtype=torch.uint8, device="cuda")
    capi.view_grid_build(dv, dw, res[0] * 4, res, grid, min_weight=1)
    field = u16_tensor(dev, n)
    ws = torch.full((capi.clearance_workspace_bytes(res),), 0xC3, dtype=torch.uint8, device="cuda")
    capi.clearance_build(grid, res, R, ub, ws, field)
    reach = torch.full((capi.reach_bytes(res) + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    capi.reach_flood(grid, field, res, r2, seeds, reach)
    out = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    capi.reach_expand(reach, res, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(Z, Y, X).astype(bool)
    want = rc.reached(states, rc.clearance(states, R, ub), r2, seeds)
    assert np.array_equal(got, want)
    return reach, want


def free_where(mask):
    return np.where(mask, rc.FREE, rc.OCCUPIED).astype(np.uint8)


def flooded_mask(dev, mask, res, seeds):
    """The reach buffer whose reached set is the part of a bool mask [Z, Y, X] that is 6-connected to `seeds` (R = 1, r2 = 1, no unknown)."""
    return flooded(dev, free_where(mask), res, 1, 0, 1, seeds)


def build_travel(dev, reach, res, seeds, limit):
    """(uint16 [Z, Y, X] on the host, the device tensor, rounds); field pre-filled with 0x5A5A, workspace with 0xC3, both guards checked,
    and the reach buffer's bytes are what they were."""
    torch, capi, _ = dev
    X, Y, Z = res
    n = X * Y * Z
    travel = u16_tensor(dev, n + GUARD)
    wsb = capi.travel_workspace_bytes()
    ws = torch.full((wsb + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    before = reach.clone()
    rounds = capi.travel_build(reach, res, seeds, limit, travel, ws)
    torch.cuda.synchronize()
    host = travel.cpu().numpy().view(np.uint16)
    assert np.all(host[n:] == 0x5A5A) and bool((ws[wsb:] == 0xC3).all()) and torch.equal(before, reach)
    return host[:n].reshape(Z, Y, X).copy(), travel, rounds


def check_travel(dev, reach, domain, res, seeds, limit):
    got, travel, rounds = build_travel(dev, reach, res, seeds, limit)
    want = tc.model(domain, seeds, limit)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (res, limit, len(bad), bad[:5], got[got != want][:5], want[got != want][:5])
    return want, travel, rounds


@pytest.mark.parametrize("res", [(20, 18, 13), (19, 18, 13)])
def test_field_equals_the_model(dev, res):
    """The random states test_reach_gpu.py floods (several components at 40 % free; a roomy scene with unknown voxels and a wider body):
    one seed, 64 at once (some impassable, some outside), an impassable seed alone, seeds outside alone; limits 0, 30 and 65534; the finite
    set is the reached set when the limit is not hit; two builds give equal bytes."""
    torch, capi, _ = dev
    X, Y, Z = res
    rng = np.random.default_rng(8)
    many = np.stack([rng.integers(-1, X + 1, 64), rng.integers(-1, Y + 1, 64), rng.integers(-1, Z + 1, 64)], axis=1)
    outside = [(-1, 3, 3), (X, 2, 2), (3, Y, 1), (2, 2, Z), (2, -5, 2)]
    cuts = []
    for states, R, ub, r2 in ((rc.random_states(res, seed=17, p=(0.3, 0.4, 0.3)), 2, 0, 1), (rc.random_states(res, seed=19, p=(0.01, 0.97, 0.02)), 3, 1, 2)):
        reach, domain = flooded(dev, states, res, R, ub, r2, many)
        assert domain.sum() > 200 and not domain.all()
        inside = [tuple(int(v) for v in p[::-1]) for p in np.argwhere(domain)]
        blocked = tuple(int(v) for v in np.argwhere(~domain)[0][::-1])
        for seeds in ([inside[len(inside) // 2]], many, [blocked], outside, [inside[0], blocked, outside[0], inside[-1], inside[0]]):
            for limit in (0, 30, 65534):
                want, _, rounds = check_travel(dev, reach, domain, res, seeds, limit)
                assert rounds >= 1 and (limit > 0 or (want != tc.NONE).sum() == len(tc.seeds_in(domain, seeds)))
            print(res, "r2", r2, "seeds", len(seeds), "finite", int((want != tc.NONE).sum()), "of", int(domain.sum()), "max", int(want[want != tc.NONE].max(initial=0)),
                  "rounds", rounds)
        want, a, _ = check_travel(dev, reach, domain, res, many, 65534)
        assert np.array_equal(want != tc.NONE, domain)                           # every flood seed is a travel seed: nothing is out of reach
        cuts.append(int((want != tc.NONE).sum() - (tc.model(domain, many, 30) != tc.NONE).sum()))
        _, b, _ = check_travel(dev, reach, domain, res, many, 65534)
        assert torch.equal(a, b)
    assert cuts[0] > 100 and min(cuts) >= 0                                      # the limit of 30 does cut the sparse scene


def test_one_tile_reaches_its_fixpoint_in_one_round(dev):
    """(8, 8, 8), one tile: a serpentine corridor one voxel wide, 20 voxels long.  One round reaches the fixpoint in LDS and one changes
    nothing: rounds == 2, which a kernel that relaxed one layer per launch would miss by far."""
    res = (8, 8, 8)
    states, path = rc.serpentine(res, z=5)
    assert len(path) >= 20
    reach, domain = flooded(dev, states, res, 1, 0, 1, [path[0]])
    assert domain.sum() == len(path)
    for seed in (path[0], path[-1], path[len(path) // 2]):
        want, _, rounds = check_travel(dev, reach, domain, res, [seed], 65534)
        assert rounds == 2 and want.max() == tc.NONE and want[want != tc.NONE].max() >= 3 * (len(path) // 2)
    want, _, rounds = check_travel(dev, reach, domain, res, [path[0]], 65534)
    assert [int(want[z, y, x]) for x, y, z in path] == [3 * i for i in range(len(path))]
    want, _, rounds = check_travel(dev, reach, domain, res, [path[0]], 0)
    assert rounds == 1 and (want != tc.NONE).sum() == 1


def test_small_thin_and_long_volumes(dev):
    """(3, 3, 3); (9, 8, 8) and (17, 9, 9), whose last tiles are one voxel wide; (300, 4, 5) all free with the seed at x = 0: values to
    3 * 299 along the axis, through 38 tiles."""
    for res in ((3, 3, 3), (9, 8, 8), (17, 9, 9)):
        X, Y, Z = res
        states = rc.random_states(res, seed=2 + X, p=(0.0, 0.8, 0.2))
        free = states == rc.FREE
        seeds = [(X - 1, int(y), int(z)) for z, y in np.argwhere(free[:, :, X - 1])[:1]] + [tuple(int(v) for v in np.argwhere(free)[0][::-1])]
        reach, domain = flooded(dev, states, res, 1, 0, 1, seeds)
        assert domain[:, :, X - 1].any() and domain.sum() > 10
        for limit in (0, 7, 65534):
            check_travel(dev, reach, domain, res, seeds, limit)
            check_travel(dev, reach, domain, res, seeds[:1], limit)
    res = (300, 4, 5)
    mask = np.ones((5, 4, 300), bool)
    reach, domain = flooded_mask(dev, mask, res, [(0, 1, 2)])
    want, _, rounds = check_travel(dev, reach, domain, res, [(0, 1, 2)], 65534)
    assert domain.all() and want[2, 1, 299] == 3 * 299 and want[0, 3, 299] == 3 * 297 + 2 * 5 and rounds >= 2
    print("(300, 4, 5): rounds", rounds)
    want, _, _ = check_travel(dev, reach, domain, res, [(0, 1, 2)], 450)
    assert want[2, 1, 150] == 450 and want[2, 1, 151] == tc.NONE


def test_corner_rule_across_tile_borders(dev):
    """(16, 16, 16): the corner move from (7, 7, 7) to (8, 8, 8) crosses the corner where eight tiles meet.  It is allowed only when all six
    intermediate voxels are in the domain: all of them, each one missing in turn, only the three face neighbours of the start, none.  The
    same for an edge move across a tile face, from (7, 3, 3) to (8, 4, 3), with both, either and neither of its two intermediates.  Both ends
    are flood seeds, so both are in the domain whether connected or not; the travel seed is the first."""
    res = (16, 16, 16)
    a, b = (7, 7, 7), (8, 8, 8)
    six = [(8, 7, 7), (7, 8, 7), (7, 7, 8), (8, 8, 7), (8, 7, 8), (7, 8, 8)]
    cases = [six] + [[v for v in six if v != miss] for miss in six] + [six[:3], []]
    costs = []
    for keep in cases:
        mask = np.zeros((16, 16, 16), bool)
        for x, y, z in [a, b] + keep:
            mask[z, y, x] = True
        reach, domain = flooded_mask(dev, mask, res, [a, b])
        assert domain.sum() == 2 + len(keep)
        want, _, _ = check_travel(dev, reach, domain, res, [a], 65534)
        costs.append(int(want[8, 8, 8]))
        back, _, _ = check_travel(dev, reach, domain, res, [b], 65534)
        assert back[7, 7, 7] == want[8, 8, 8]
    print("corner move: cost of (8, 8, 8) per case", costs)
    assert costs[0] == 5 and all(5 < c < tc.NONE for c in costs[1:7]) and costs[7] == tc.NONE and costs[8] == tc.NONE
    a, b = (7, 3, 3), (8, 4, 3)
    two = [(8, 3, 3), (7, 4, 3)]
    costs = []
    for keep in (two, two[:1], two[1:], []):
        mask = np.zeros((16, 16, 16), bool)
        for x, y, z in [a, b] + keep:
            mask[z, y, x] = True
        reach, domain = flooded_mask(dev, mask, res, [a, b])
        want, _, _ = check_travel(dev, reach, domain, res, [a], 65534)
        costs.append(int(want[3, 4, 8]))
    assert costs == [4, 6, 6, tc.NONE]
    # a block of free space around the corner: every move direction crosses some tile border
    mask = np.zeros((16, 16, 16), bool)
    mask[5:11, 5:11, 5:11] = np.random.default_rng(5).random((6, 6, 6)) < 0.8
    seed = tuple(int(v) for v in np.argwhere(mask)[0][::-1])
    reach, domain = flooded_mask(dev, mask, res, [seed])
    assert domain.sum() > 100
    check_travel(dev, reach, domain, res, [seed], 65534)


def test_serpentine_across_tiles(dev):
    """The flood test's serpentine on (20, 18, 13): it crosses tile faces and doubles back through tiles it has left, so several rounds are
    needed; the cost is three per voxel walked.  At the full limit and at one that cuts it half way."""
    res = (20, 18, 13)
    states, path = rc.serpentine(res)
    tiles = [tuple(c >> 3 for c in v) for v in path]
    crossings = sum(1 for p, q in zip(tiles[:-1], tiles[1:]) if p != q)
    assert crossings >= 15 and len(set(tiles[:18]) & set(tiles[19:37])) >= 2
    reach, domain = flooded(dev, states, res, 1, 0, 1, [path[0]])
    want, _, rounds = check_travel(dev, reach, domain, res, [path[0]], 65534)
    print("serpentine: voxels", len(path), "tile faces crossed", crossings, "rounds", rounds)
    assert [int(want[z, y, x]) for x, y, z in path] == [3 * i for i in range(len(path))] and 2 < rounds <= crossings + 2
    half = 3 * (len(path) // 2)
    want, _, _ = check_travel(dev, reach, domain, res, [path[0]], half)
    assert [int(want[z, y, x]) for x, y, z in path] == [3 * i if 3 * i <= half else tc.NONE for i in range(len(path))]
    want, _, _ = check_travel(dev, reach, domain, res, [path[-1], path[len(path) // 2]], 65534)
    assert want[path[0][2], path[0][1], path[0][0]] == 3 * (len(path) // 2)


@pytest.fixture(scope="module")
def scene(dev):
    """The path and query tests' inputs, computed once: a roomy random scene on (19, 18, 13) flooded from two seeds, its field at limit 40, which leaves a third of the reached voxels beyond it."""
    res = (19, 18, 13)
    states = rc.random_states(res, seed=29, p=(0.0, 0.8, 0.2))
    free = np.argwhere(states == rc.FREE)
    seeds = [tuple(int(v) for v in free[0][::-1]), tuple(int(v) for v in free[len(free) // 3][::-1])]
    reach, domain = flooded(dev, states, res, 1, 0, 1, seeds)
    limit = 40
    want, travel, _ = check_travel(dev, reach, domain, res, seeds, limit)
    assert domain.sum() > 1000 and 0 < ((want == tc.NONE) & domain).sum()
    return dict(res=res, reach=reach, domain=domain, seeds=seeds, limit=limit, travel=travel, want=want)


def test_paths_equal_the_model(dev, scene):
    """64 targets at once: both seeds, unreached voxels, voxels outside the volume, voxels beyond the limit and reached voxels near and far.
    With a capacity larger than every path and with capacity 3: the lengths are full either way, slots beyond a path's end (or beyond the
    capacity) are untouched."""
    torch, capi, _ = dev
    res, domain, want = scene["res"], scene["domain"], scene["want"]
    X, Y, Z = res
    finite = [tuple(int(v) for v in p[::-1]) for p in np.argwhere(want != tc.NONE)]
    far = sorted(finite, key=lambda v: -int(want[v[2], v[1], v[0]]))[:20]
    beyond = [tuple(int(v) for v in p[::-1]) for p in np.argwhere((want == tc.NONE) & domain)[:4]]
    blocked = [tuple(int(v) for v in p[::-1]) for p in np.argwhere(~domain)[:4]]
    outside = [(-1, 3, 3), (X, 2, 2), (3, Y, 1), (2, 2, Z), (2, -5, 2), (1 << 30, 0, 0)]
    targets = (scene["seeds"] + blocked + outside + beyond + far + finite[:: max(1, len(finite) // 28)])[:64]
    assert len(targets) == 64
    paths = [tc.walk(want, domain, t) for t in targets]
    longest = max(len(p) for p in paths)
    assert longest >= 10 and sum(1 for p in paths if not p) == 14 and [len(p) for p in paths[:2]] == [1, 1]
    dt = torch.from_numpy(np.array(targets, np.int32).reshape(-1)).cuda()
    for n, capacity in ((64, longest + 5), (64, 3), (1, 1), (37, longest)):
        out = torch.full((n * capacity * 3 + GUARD,), -77, dtype=torch.int32, device="cuda")
        lens = torch.full((n + GUARD,), -77, dtype=torch.int32, device="cuda")
        capi.travel_path(n, dt, res, scene["reach"], scene["travel"], scene["limit"], capacity, out, lens)
        torch.cuda.synchronize()
        o, l = out.cpu().numpy(), lens.cpu().numpy()
        assert np.all(o[n * capacity * 3:] == -77) and np.all(l[n:] == -77)
        assert [int(v) for v in l[:n]] == [len(p) for p in paths[:n]]
        o = o[:n * capacity * 3].reshape(n, capacity, 3)
        for i in range(n):
            k = min(len(paths[i]), capacity)
            assert [tuple(int(c) for c in v) for v in o[i, :k]] == paths[i][:k], (i, targets[i])
            assert np.all(o[i, k:] == -77)


def test_queries_equal_the_field(dev, scene):
    """Voxels inside the volume answer with the field's value (NONE among them), voxels outside with NONE."""
    torch, capi, _ = dev
    X, Y, Z = scene["res"]
    rng = np.random.default_rng(41)
    v = np.stack([rng.integers(-2, X + 2, 300), rng.integers(-2, Y + 2, 300), rng.integers(-2, Z + 2, 300)], axis=1).astype(np.int32)
    v[:4] = [(-1, -1, -1), (X - 1, Y - 1, Z - 1), (0, 0, 0), (-2 ** 31, 2 ** 31 - 1, 0)]
    inside = (v[:, 0] >= 0) & (v[:, 0] < X) & (v[:, 1] >= 0) & (v[:, 1] < Y) & (v[:, 2] >= 0) & (v[:, 2] < Z)
    want = np.full(300, tc.NONE, np.uint16)
    want[inside] = scene["want"][v[inside, 2], v[inside, 1], v[inside, 0]]
    assert 0 < inside.sum() < 300 and len(np.unique(want)) > 10
    out = u16_tensor(dev, 300 + GUARD)
    capi.travel_query(300, torch.from_numpy(v.reshape(-1)).cuda(), scene["res"], scene["travel"], out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[:300], want) and np.all(got[300:] == 0x5A5A)


def test_argument_checks(dev, scene):
    """Every refused call returns hipErrorInvalidValue (XsError) and leaves its outputs untouched."""
    torch, capi, _ = dev
    res = scene["res"]
    n = res[0] * res[1] * res[2]
    reach, good = scene["reach"], scene["travel"]
    travel = u16_tensor(dev, n)
    ws = torch.full((capi.travel_workspace_bytes(),), 0xC3, dtype=torch.uint8, device="cuda")
    one = [(3, 3, 3)]
    for kw in (dict(seeds=np.zeros((0, 3), np.int32)), dict(seeds=np.zeros((65, 3), np.int32)), dict(limit=-1), dict(limit=65535), dict(limit=1 << 20),
               dict(res=(0, 18, 13)), dict(res=(19, 18, -1)), dict(res=(19, 70000, 13)), dict(reach=None), dict(travel=None), dict(workspace=None)):
        a = dict(reach=reach, res=res, seeds=one, limit=30, travel=travel, workspace=ws)
        a.update(kw)
        with pytest.raises(capi.XsError):
            capi.travel_build(**a)
    torch.cuda.synchronize()
    assert bool((travel.view(torch.uint8) == 0x5A).all()) and bool((ws == 0xC3).all())
    vox = torch.zeros(3 * 8, dtype=torch.int32, device="cuda")
    out = u16_tensor(dev, 8)
    for kw in (dict(n=0), dict(n=-3), dict(res=(19, 18, 0)), dict(voxels=None), dict(travel=None), dict(out=None)):
        a = dict(n=8, voxels=vox, res=res, travel=good, out=out)
        a.update(kw)
        with pytest.raises(capi.XsError):
            capi.travel_query(**a)
    path = torch.full((8 * 4 * 3,), -77, dtype=torch.int32, device="cuda")
    lens = torch.full((8,), -77, dtype=torch.int32, device="cuda")
    for kw in (dict(n=0), dict(n=65), dict(capacity=0), dict(capacity=-1), dict(limit=-1), dict(limit=65535), dict(res=(19, 0, 13)), dict(targets=None),
               dict(reach=None), dict(travel=None), dict(path=None), dict(lengths=None)):
        a = dict(n=8, targets=vox, res=res, reach=reach, travel=good, limit=30, capacity=4, path=path, lengths=lens)
        a.update(kw)
        with pytest.raises(capi.XsError):
            capi.travel_path(**a)
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == 0x5A).all()) and bool((path == -77).all()) and bool((lens == -77).all())
    capi.travel_path(8, vox, res, reach, good, 65534, 1, path, lens)              # the edges of the valid ranges do launch
    capi.travel_query(1, vox, res, good, out)
    torch.cuda.synchronize()
    assert bool((lens >= 0).all())


# ---- orchestrator level ----------------------------------------------------------------------------------------------------------------
# The setting of test_reach_gpu.py's orchestrator test: scene S3 at 64^3, four frames, 64 pose_candidates within +-0.3 m and +-0.3 rad of
# the last pose, a body of 0.1 m; a voxel is 0.12 m.
ORCH_BOX_T, ORCH_RADIUS = 0.3, 0.1


def model_of_kf(kf, prm, cands, radius_m, snap, unknown_blocks, max_travel_m=None):
    n = kf.res[0]
    v, w, _ = kf.volume()
    states = vc.states_of(v.reshape(n, n, n), w.reshape(n, n, n), 1)
    vs = prm["tsdf_voxel_size"]
    r2, R = rc.radius_of(radius_m, vs)
    field = rc.clearance(states, R, unknown_blocks)
    passable = rc.passable_of(states, field, r2)
    found, _, seed = rc.query(np.asarray(kf.camera2volume(), np.float32)[:3, 3, 0][None], vs, passable, field, snap)
    assert found[0]
    reached = rc.reached(states, field, r2, seed)
    flags, clear2, voxel = rc.query(cands[:, :3, 3, 0], vs, reached, field, 0)
    limit = tc.travel_limit(0.0 if max_travel_m is None else max_travel_m, vs)
    travel = tc.model(reached, seed, limit)
    cost = np.array([travel[z, y, x] if f else tc.NONE for f, (x, y, z) in zip(flags, voxel)], np.uint16)
    metres = np.where(cost == tc.NONE, np.inf, cost.astype(np.float64) * float(np.float32(vs)) / 3.0)
    return dict(reached=reached, seed=tuple(int(c) for c in seed[0]), flags=flags.astype(bool), clear2=clear2, voxel=voxel, travel=travel, cost=cost, metres=metres,
                limit=limit, vs=np.float32(vs))


def test_orchestrator_follows_the_volume(dev):
    """travel equals the model on the downloaded volume(), also with max_travel_m set so that a reachable candidate falls beyond it; path_to
    of a reachable candidate is the model's path reversed with points at voxel centres, of an unreachable one None; next_view_by_travel is
    the model's pick; next_reachable_view, next_best_view and reachable return what they returned before the new calls ran; after one more
    frame everything is rebuilt and equals the model again."""
    torch, capi, pl = dev
    n = 64
    prm = synth.s1_params(n)
    kf = pl.KinectFusion(prm)
    dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(5)]
    for k in range(4):
        assert kf.process_frame(dfr[k]) == 1
    cands = pl.pose_candidates(kf.camera2volume(), ORCH_BOX_T, 0.3, 64)
    before = dict(best=kf.next_best_view(cands), reach=kf.reachable(cands, ORCH_RADIUS), nrv=kf.next_reachable_view(cands, ORCH_RADIUS))

    def check(tag):
        m = model_of_kf(kf, prm, cands, ORCH_RADIUS, 4, 1)
        flags, clear2, metres = kf.travel(cands, ORCH_RADIUS)
        print(tag, "seed", m["seed"], "reached voxels", int(m["reached"].sum()), "reachable candidates", int(m["flags"].sum()), "costs",
              sorted(int(c) for c in m["cost"][m["flags"]]))
        assert 0 < m["flags"].sum() < 64 and np.array_equal(m["cost"] != tc.NONE, m["flags"])
        assert flags.dtype == bool and np.array_equal(flags, m["flags"]) and np.array_equal(clear2, m["clear2"])
        assert metres.dtype == np.float64 and np.array_equal(metres, m["metres"])
        # a limit between the nearest and the farthest reachable candidate
        costs = np.unique(m["cost"][m["flags"]])
        assert len(costs) >= 2
        cut_m = float(costs[0] + costs[-1]) / 2.0 * float(m["vs"]) / 3.0
        mc = model_of_kf(kf, prm, cands, ORCH_RADIUS, 4, 1, max_travel_m=cut_m)
        assert (mc["flags"] & (mc["cost"] == tc.NONE)).any() and (mc["cost"] != tc.NONE).any() and mc["limit"] < 65534
        f2, c2, m2 = kf.travel(cands, ORCH_RADIUS, max_travel_m=cut_m)
        assert np.array_equal(f2, mc["flags"]) and np.array_equal(c2, mc["clear2"]) and np.array_equal(m2, mc["metres"])
        again = kf.travel(cands, ORCH_RADIUS)                                    # (rebuilt at the full limit)
        assert np.array_equal(again[2], m["metres"])
        # paths
        far = int(np.argmax(np.where(m["flags"], m["cost"], 0)))
        want = tc.walk(m["travel"], m["reached"], m["voxel"][far])[::-1]
        assert len(want) >= 2 and want[0] == m["seed"]
        for capacity in (1024, 1):                                               # (capacity 1: the retry with the needed capacity)
            points, voxels = kf.path_to(cands[far], ORCH_RADIUS, capacity=capacity)
            assert voxels.dtype == np.int32 and points.dtype == np.float32 and [tuple(int(c) for c in v) for v in voxels] == want
            assert np.array_equal(points, (voxels.astype(np.float32) + np.float32(0.5)) * m["vs"])
        assert kf.path_to(cands[int(np.flatnonzero(~m["flags"])[0])], ORCH_RADIUS) is None
        beyond = int(np.flatnonzero(mc["flags"] & (mc["cost"] == tc.NONE))[0])
        assert kf.path_to(cands[beyond], ORCH_RADIUS, max_travel_m=cut_m) is None and kf.path_to(cands[beyond], ORCH_RADIUS) is not None
        # the selection
        best_counts = kf.next_best_view(cands)[1]
        for bias_m, hits in ((0.5, None), (0.5, 0), (0.01, 0), (50.0, 0)):
            pick, counts, tm = kf.next_view_by_travel(cands, ORCH_RADIUS, bias_m=bias_m, min_hits=hits)
            want_pick = tc.next_view_by_travel(best_counts, m["cost"], 80 * 60 // 4 if hits is None else hits, tc.travel_bias(bias_m, m["vs"]))
            assert pick == want_pick and np.array_equal(counts, best_counts) and np.array_equal(tm, m["metres"]), (bias_m, hits)
            assert pick < 0 or m["flags"][pick]
        assert kf.next_view_by_travel(cands, ORCH_RADIUS, min_hits=0)[0] >= 0 and kf.next_view_by_travel(cands, ORCH_RADIUS, min_hits=10 ** 9)[0] == -1
        return m

    m = check("after four frames:")
    # what was there before answers as before
    best, reach, nrv = kf.next_best_view(cands), kf.reachable(cands, ORCH_RADIUS), kf.next_reachable_view(cands, ORCH_RADIUS)
    assert best[0] == before["best"][0] and np.array_equal(best[1], before["best"][1])
    assert np.array_equal(reach[0], before["reach"][0]) and np.array_equal(reach[1], before["reach"][1])
    assert nrv[0] == before["nrv"][0] and np.array_equal(nrv[1], before["nrv"][1]) and np.array_equal(nrv[2], before["nrv"][2])
    for bad in (dict(radius_m=40.0), dict(radius_m=-1.0), dict(radius_m=ORCH_RADIUS, snap_vox=17), dict(radius_m=ORCH_RADIUS, max_travel_m=float("nan"))):
        with pytest.raises(ValueError):
            kf.travel(cands, **bad)
        with pytest.raises(ValueError):
            kf.path_to(cands[0], **bad)
    with pytest.raises(ValueError):
        kf.next_view_by_travel(cands, 40.0)
    with pytest.raises(ValueError):
        kf.next_view_by_travel(cands, ORCH_RADIUS, bias_m=-1.0)
    assert kf.process_frame(dfr[4]) == 1
    m2 = check("after one more frame:")
    assert (m2["travel"] != m["travel"]).any()
    kf.close()


def test_shard_mode_refuses(dev):
    """Two ranks as threads on one GPU: travel, path_to and next_view_by_travel raise XsError on every rank and do nothing, and the pipeline
    tracks the next frame afterwards."""
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
            for call in (lambda: shards[r].travel(cands, 0.06), lambda: shards[r].path_to(cands[0], 0.06), lambda: shards[r].next_view_by_travel(cands, 0.06)):
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
