"""GPU: the frontier mask (xs_frontier_mask), its cluster labels (xs_frontier_label), the cluster records (xs_frontier_clusters) and the
orchestrator's calls built on them (KinectFusion.frontiers, propose_views, explore_step); DESIGN.md section 4.21.  Everything but the
proposed poses is integer arithmetic, so every comparison is for EQUALITY with the scipy model of tests/frontier_cases.py; the poses carry
bounds derived from their operation count.  Outputs are pre-filled with garbage and carry a guard; the grid's bytes are unchanged."""
import importlib
import threading

import numpy as np
import pytest

import frontier_cases as fc
import reach_cases as rc
import travel_cases as tc
import view_cases as vc
from helpers import synth

pytestmark = pytest.mark.gpu
GUARD = 64
EPS = 2.0 ** -24                                                               # the relative error of one float32 rounding


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


def grid_of(dev, states, res):
    """The observation grid of a state array [Z, Y, X], built on the GPU into a buffer pre-filled with 0xA5 (so padding bits are garbage
    wherever the build leaves them alone)."""
    torch, capi, _ = dev
    value, weight = vc.volumes_of(states)
    dv = torch.from_numpy(np.ascontiguousarray(value, np.float32).reshape(-1)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(weight, np.int32).reshape(-1)).cuda()
    grid = torch.full((capi.view_grid_bytes(res),), 0xA5, dtype=torch.uint8, device="cuda")
    capi.view_grid_build(dv, dw, res[0] * 4, res, grid, min_weight=1)
    return grid


def run_frontier(dev, grid, res, cell):
    """One pass through the four calls.  Returns dict(mask bool [Z, Y, X], labels uint32 [Z, Y, X], records uint64 [n, 8], rounds, and the
    raw device tensors for byte comparisons).  Checks on the way: every guard, the grid's bytes, the mask's overhang bits, the count at a
    capacity below it with the records untouched."""
    torch, capi, _ = dev
    X, Y, Z = res
    n = X * Y * Z
    before = grid.clone()
    mb, lb = capi.frontier_mask_bytes(res), capi.frontier_label_bytes(res)
    assert mb > 0 and lb == 4 * n
    mask = torch.full((mb + GUARD,), 0xEE, dtype=torch.uint8, device="cuda")
    capi.frontier_mask(grid, res, mask)
    out = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    capi.frontier_expand(mask, res, out)
    labels = torch.full((n + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    wsb = capi.frontier_workspace_bytes(res, 0)
    ws = torch.full((wsb + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
    rounds = capi.frontier_label(mask, res, cell, labels, ws)
    torch.cuda.synchronize()
    assert bool((mask[mb:] == 0xEE).all()) and bool((out[n:] == 0x77).all()) and bool((labels[n:] == 0x5A5A5A5A).all()) and bool((ws[wsb:] == 0xC3).all())
    m = out[:n].cpu().numpy().reshape(Z, Y, X)
    assert set(np.unique(m)) <= {0, 1}
    # every set bit of the mask words is a voxel inside the volume: the expanded bytes account for all of them
    words = mask[:mb].cpu().numpy().view(np.uint64)
    assert int(sum(bin(int(w)).count("1") for w in words)) == int(m.sum())
    lab = labels[:n].cpu().numpy().view(np.uint32).reshape(Z, Y, X)

    def clusters(capacity):
        rec = torch.full((capacity * 8 + GUARD,), -77, dtype=torch.int64, device="cuda")
        cnt = torch.full((1 + GUARD,), -77, dtype=torch.int32, device="cuda")
        wb = capi.frontier_workspace_bytes(res, capacity)
        w = torch.full((wb + GUARD,), 0xC3, dtype=torch.uint8, device="cuda")
        got = capi.frontier_clusters(mask, labels, res, capacity, rec, cnt, w)
        torch.cuda.synchronize()
        assert int(cnt[0]) == got and bool((cnt[1:] == -77).all()) and bool((rec[capacity * 8:] == -77).all()) and bool((w[wb:] == 0xC3).all())
        return got, rec

    count, rec = clusters(1)
    if count > 1:
        assert bool((rec == -77).all())                                          # capacity 1 < count: the count alone
        c2, rec = clusters(count - 1)
        assert c2 == count and bool((rec == -77).all())
        c3, rec = clusters(count)
        assert c3 == count
    elif count == 0:
        assert bool((rec == -77).all())
    torch.cuda.synchronize()
    assert torch.equal(before, grid)
    records = rec[:count * 8].cpu().numpy().view(np.uint64).reshape(count, 8).copy()
    return dict(mask=m.astype(bool), labels=lab.copy(), records=records, rounds=rounds, d_mask=mask, d_labels=labels, d_records=rec)


def check_case(dev, states, res, cell, grid=None):
    """The three results equal the model; two runs give equal bytes."""
    torch = dev[0]
    grid = grid_of(dev, states, res) if grid is None else grid
    want_m, want_lab, want_rec = fc.model(states, cell)
    a = run_frontier(dev, grid, res, cell)
    assert np.array_equal(a["mask"], want_m), (res, cell, np.argwhere(a["mask"] != want_m)[:5])
    bad = np.argwhere(a["labels"] != want_lab)
    assert len(bad) == 0, (res, cell, len(bad), bad[:5], a["labels"][a["labels"] != want_lab][:5], want_lab[a["labels"] != want_lab][:5])
    assert a["records"].shape == want_rec.shape and np.array_equal(a["records"], want_rec), (res, cell, a["records"][:3], want_rec[:3])
    b = run_frontier(dev, grid, res, cell)
    assert torch.equal(a["d_mask"], b["d_mask"]) and torch.equal(a["d_labels"], b["d_labels"]) and torch.equal(a["d_records"], b["d_records"])
    assert a["rounds"] >= 1
    return a


@pytest.mark.parametrize("res", [(20, 18, 13), (19, 18, 13)])
def test_random_scenes_equal_the_model(dev, res):
    """The two random scenes of the issue (a roomy one with sparse unknown voxels: some 270 frontier voxels in two dozen clusters; a dense
    one whose 1 600 frontier voxels percolate into two clusters) at cell 0, 8 and 16: mask, labels and records equal the model, two runs
    give equal bytes, a capacity below the count returns the count alone.  More than one cluster, and more at cell 8 than at cell 0."""
    for seed, p in ((19, (0.01, 0.97, 0.02)), (17, (0.3, 0.4, 0.3))):
        states = rc.random_states(res, seed=seed, p=p)
        grid = grid_of(dev, states, res)
        n = {}
        for cell in (0, 8, 16):
            a = check_case(dev, states, res, cell, grid)
            n[cell] = len(a["records"])
            print(res, "seed", seed, "cell", cell, "frontier", int(a["mask"].sum()), "clusters", n[cell], "rounds", a["rounds"])
        assert n[0] > 1 and n[8] > n[0] and n[8] >= n[16] >= n[0]


def test_one_tile_reaches_its_fixpoint_in_one_round(dev):
    """(8, 8, 8), one tile: the serpentine corridor of the flood tests in plane z = 5 under an UNKNOWN plane z = 6.  Its 20 voxels are the
    whole frontier and one cluster along the path (the runs are two voxels apart).  One round reaches the fixpoint in LDS and one changes
    nothing: rounds == 2, which a kernel that moved a label one voxel per launch would miss by far."""
    res = (8, 8, 8)
    states, path = rc.serpentine(res, z=5)
    states[6] = fc.UNKNOWN
    a = check_case(dev, states, res, 0)
    assert len(path) == 20 and a["mask"].sum() == 20 and all(a["mask"][z, y, x] for x, y, z in path)
    x, y, z = path[0]
    assert len(a["records"]) == 1 and a["records"][0, 0] == (z * 8 + y) * 8 + x and a["records"][0, 1] == 20 and a["rounds"] == 2
    assert check_case(dev, states, res, 8)["rounds"] == 2


def test_small_and_thin_volumes(dev):
    """(3, 3, 3); (9, 8, 8) and (17, 9, 9), whose last tiles are one voxel wide; (5, 5, 5) all FREE: no frontier (overhang padding and the
    outside are not UNKNOWN); (300, 4, 5), FREE for y < 2 and UNKNOWN above: the 1 500 voxels of plane y = 1, one cluster labelled 300 at cell
    0 through 38 tiles, split by cell along x at cell 8."""
    for res in ((3, 3, 3), (9, 8, 8), (17, 9, 9)):
        for seed, p in ((2 + res[0], (0.2, 0.7, 0.1)), (5, (0.5, 0.5, 0.0))):
            states = rc.random_states(res, seed=seed, p=p)
            for cell in (0, 8):
                a = check_case(dev, states, res, cell)
                assert a["mask"].sum() > 3
        # the last plane along x alone: FREE there, UNKNOWN in the plane before it
        states = np.full(res[::-1], fc.OCCUPIED, np.uint8)
        states[:, :, -1], states[:, :, -2] = fc.FREE, fc.UNKNOWN
        a = check_case(dev, states, res, 8)
        assert a["mask"][:, :, -1].all() and a["mask"].sum() == res[1] * res[2]
    res = (5, 5, 5)
    a = check_case(dev, np.full((5, 5, 5), fc.FREE, np.uint8), res, 0)
    assert not a["mask"].any() and len(a["records"]) == 0 and a["rounds"] == 1 and np.all(a["labels"] == fc.NONE)
    res = (300, 4, 5)
    states = np.full((5, 4, 300), fc.UNKNOWN, np.uint8)
    states[:, :2, :] = fc.FREE
    a = check_case(dev, states, res, 0)
    assert a["mask"].sum() == 1500 and a["mask"][:, 1, :].all() and len(a["records"]) == 1 and a["records"][0, 0] == 300 and a["records"][0, 1] == 1500
    assert fc.unpack_box(a["records"][0, 5]) == (0, 1, 0) and fc.unpack_box(a["records"][0, 6]) == (299, 1, 4) and a["rounds"] > 2
    print("(300, 4, 5): rounds", a["rounds"])
    b = check_case(dev, states, res, 8)
    assert len(b["records"]) == 38 and [int(r) for r in b["records"][:, 0]] == [300 + 8 * k for k in range(38)] and b["rounds"] == 2


def test_across_a_tile_corner(dev):
    """(16, 16, 16): frontier voxels at (7, 7, 7) and (8, 8, 8) — each a FREE voxel with one UNKNOWN face neighbour in an OCCUPIED volume —
    are one cluster at cell 0 and 16, across the corner where eight tiles meet, and two at cell 8.  A pair two voxels apart is always two."""
    res = (16, 16, 16)
    for b, want in (((8, 8, 8), {0: 1, 8: 2, 16: 1}), ((9, 9, 9), {0: 2, 8: 2, 16: 2}), ((8, 7, 6), {0: 1, 8: 2, 16: 1})):
        states = np.full((16, 16, 16), fc.OCCUPIED, np.uint8)
        states[7, 7, 7], states[6, 7, 7] = fc.FREE, fc.UNKNOWN                   # (x, y, z) = (7, 7, 7) with the unknown below it
        states[b[2], b[1], b[0]], states[b[2] + 1, b[1], b[0]] = fc.FREE, fc.UNKNOWN
        grid = grid_of(dev, states, res)
        for cell in (0, 8, 16):
            a = check_case(dev, states, res, cell, grid)
            assert a["mask"].sum() == 2 and a["mask"][7, 7, 7] and a["mask"][b[2], b[1], b[0]]
            assert len(a["records"]) == want[cell], (b, cell)
            if want[cell] == 1:
                assert a["records"][0, 0] == min((7 * 16 + 7) * 16 + 7, (b[2] * 16 + b[1]) * 16 + b[0]) and a["records"][0, 1] == 2


def test_argument_checks(dev):
    """Every refused call returns hipErrorInvalidValue (XsError) and leaves its outputs untouched."""
    torch, capi, _ = dev
    res = (19, 18, 13)
    n = res[0] * res[1] * res[2]
    states = rc.random_states(res, seed=19, p=(0.01, 0.97, 0.02))
    grid = grid_of(dev, states, res)
    good = run_frontier(dev, grid, res, 8)
    mask = torch.full((capi.frontier_mask_bytes(res),), 0xEE, dtype=torch.uint8, device="cuda")
    out = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    labels = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    ws = torch.full((capi.frontier_workspace_bytes(res, 64),), 0xC3, dtype=torch.uint8, device="cuda")
    rec = torch.full((64 * 8,), -77, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), -77, dtype=torch.int32, device="cuda")
    bad_res = ((0, 18, 13), (19, 18, -1), (19, 70000, 13), (2048, 2048, 1024))
    for kw in [dict(res=r) for r in bad_res] + [dict(grid=None), dict(mask=None)]:
        a = dict(grid=grid, res=res, mask=mask)
        a.update(kw)
        with pytest.raises(capi.XsError):
            capi.frontier_mask(**a)
    for kw in [dict(res=r) for r in bad_res] + [dict(mask=None), dict(out=None)]:
        a = dict(mask=good["d_mask"], res=res, out=out)
        a.update(kw)
        with pytest.raises(capi.XsError):
            capi.frontier_expand(**a)
    for kw in [dict(res=r) for r in bad_res] + [dict(cell=c) for c in (-8, 1, 4, 12, 65536, 1 << 20)] + [dict(mask=None), dict(labels=None), dict(workspace=None)]:
        a = dict(mask=good["d_mask"], res=res, cell=8, labels=labels, workspace=ws)
        a.update(kw)
        with pytest.raises(capi.XsError):
            capi.frontier_label(**a)
    for kw in [dict(res=r) for r in bad_res] + [dict(capacity=0), dict(capacity=-5), dict(mask=None), dict(labels=None), dict(records=None), dict(count=None),
                                                dict(workspace=None)]:
        a = dict(mask=good["d_mask"], labels=good["d_labels"], res=res, capacity=64, records=rec, count=cnt, workspace=ws)
        a.update(kw)
        with pytest.raises(capi.XsError):
            capi.frontier_clusters(**a)
    torch.cuda.synchronize()
    assert bool((mask == 0xEE).all()) and bool((out == 0x77).all()) and bool((labels == 0x5A5A5A5A).all()) and bool((ws == 0xC3).all())
    assert bool((rec == -77).all()) and bool((cnt == -77).all())
    assert capi.frontier_label(good["d_mask"], res, 65528, labels, ws) >= 1           # the edges of the valid ranges do launch
    assert capi.frontier_clusters(good["d_mask"], labels, res, 64, rec, cnt, ws) == len(fc.model(states, 0)[2])


# ---- orchestrator level ----------------------------------------------------------------------------------------------------------------
# The setting of test_reach_gpu.py's and test_travel_gpu.py's orchestrator tests: scene S3 at 64^3, four tracked frames, a body of 0.1 m; a
# voxel is 0.12 m.
ORCH_BOX_T, ORCH_RADIUS, ORCH_SNAP = 0.3, 0.1, 4
ORCH_CELL, ORCH_MIN_SIZE, ORCH_VIEWS, ORCH_STANDOFF = 32, 8, 6, 1.0


def world_model(kf, prm):
    """The states of the downloaded volume, the model's flood from the snapped camera and its travel field."""
    n = kf.res[0]
    v, w, _ = kf.volume()
    states = vc.states_of(v.reshape(n, n, n), w.reshape(n, n, n), 1)
    vs = prm["tsdf_voxel_size"]
    r2, R = rc.radius_of(ORCH_RADIUS, vs)
    field = rc.clearance(states, R, 1)
    passable = rc.passable_of(states, field, r2)
    found, _, seed = rc.query(np.asarray(kf.camera2volume(), np.float32)[:3, 3, 0][None], vs, passable, field, ORCH_SNAP)
    assert found[0]
    reached = rc.reached(states, field, r2, seed)
    return dict(states=states, field=field, reached=reached, seed=seed, vs=np.float32(vs), travel=tc.model(reached, seed, 65534))


def model_proposals(w, rec, cam):
    """The (cluster, voxel) pairs the contract yields, in order: the numpy twins of view_host.hpp and reach_cases' snap rule."""
    pairs = []
    for i, r in enumerate(rec):
        c = fc.centroid(r, w["vs"])
        pts = np.stack([(c + np.float32(ORCH_STANDOFF) * fc.direction(j).astype(np.float32)).astype(np.float32) for j in range(ORCH_VIEWS)])
        found, _, voxel = rc.query(pts, w["vs"], w["reached"], w["field"], ORCH_SNAP)
        seen = set()
        for f, v in zip(found, voxel):
            v = tuple(int(t) for t in v)
            if f and v not in seen:
                seen.add(v)
                pairs.append((i, v))
    return pairs


def test_orchestrator_follows_the_volume(dev):
    """frontiers equals the model on the downloaded volume(); every pose of propose_views sits at the centre of a voxel the model's flood
    reaches, looks at its cluster's centroid within the derived bound and comes from a cluster of at least min_size voxels, and the
    (cluster, voxel) pairs are the model's; reachable says yes for all of them, more than the 3 of 64 pose_candidates yields; explore_step's
    pick is the model's next_view_by_travel pick over the same candidates and its path is path_to's; after one more frame everything is
    rebuilt; the earlier calls return what they returned before.

    Pose bounds (EPS = 2^-24): the rotation is built in float64 and rounded once per entry, so R^T R is the identity within 8 EPS and the
    optical axis is parallel to centroid - position within 2 EPS, as in tests/cxx/frontier_selftest.cpp; the test forms centroid - position
    from the float32 values the library used, in float64."""
    torch, capi, pl = dev
    n = 64
    prm = synth.s1_params(n)
    kf = pl.KinectFusion(prm)
    dfr = [torch.from_numpy(synth.s3_frame(k).view(np.int16)).cuda() for k in range(5)]
    for k in range(4):
        assert kf.process_frame(dfr[k]) == 1
    old = pl.pose_candidates(kf.camera2volume(), ORCH_BOX_T, 0.3, 64)
    before = dict(best=kf.next_best_view(old), reach=kf.reachable(old, ORCH_RADIUS), travel=kf.travel(old, ORCH_RADIUS), pick=kf.next_view_by_travel(old, ORCH_RADIUS))
    assert int(before["reach"][0].sum()) == 3

    def check(tag):
        w = world_model(kf, prm)
        m, lab, rec = fc.model(w["states"], ORCH_CELL)
        keep = rec[rec[:, 1] >= ORCH_MIN_SIZE]
        got = kf.frontiers(ORCH_CELL, ORCH_MIN_SIZE)
        assert len(keep) > 1 and len(got) == len(keep)
        median = int(np.median(rec[:, 1])) + 1                                   # a size that drops some clusters and keeps others
        fewer = kf.frontiers(ORCH_CELL, median)
        assert 0 < len(fewer) < len(rec) and np.array_equal(fewer["label"], rec[rec[:, 1] >= median][:, 0].astype(np.uint32))
        assert np.array_equal(got["label"], keep[:, 0].astype(np.uint32)) and np.array_equal(got["count"], keep[:, 1]) and np.array_equal(got["sum"], keep[:, 2:5])
        assert np.array_equal(got["centroid"], np.stack([fc.centroid(r, w["vs"]) for r in keep]))
        assert [tuple(v) for v in got["min"]] == [fc.unpack_box(r[5]) for r in keep] and [tuple(v) for v in got["max"]] == [fc.unpack_box(r[6]) for r in keep]
        every = kf.frontiers(ORCH_CELL, 0)
        assert np.array_equal(every["label"], rec[:, 0].astype(np.uint32)) and int(every["count"].sum()) == int(m.sum())
        whole = kf.frontiers(0, 0)                                               # another cell size: rebuilt
        assert np.array_equal(whole["label"], fc.model(w["states"], 0)[2][:, 0].astype(np.uint32)) and len(whole) <= len(every)
        # the proposed views
        cands, cluster = kf.propose_views(ORCH_RADIUS, ORCH_VIEWS, ORCH_STANDOFF, ORCH_CELL, ORCH_MIN_SIZE, ORCH_SNAP, ORCH_SNAP)
        P = len(cands)
        print(tag, "frontier voxels", int(m.sum()), "clusters", len(rec), "kept", len(keep), "reached voxels", int(w["reached"].sum()), "proposed", P)
        assert cands.dtype == np.float32 and cands.shape == (P, 4, 4, 2) and cluster.dtype == np.int32 and P > 3
        assert not cands[..., 1].any() and np.array_equal(cands[:, 3, :, 0], np.tile(np.array([0, 0, 0, 1], np.float32), (P, 1)))
        pos = cands[:, :3, 3, 0]
        voxel = np.floor(pos / w["vs"]).astype(np.int64)
        assert np.array_equal(pos, fc.voxel_centre(voxel, w["vs"]))              # at a voxel's centre, and the centre gives the voxel back
        assert all(w["reached"][z, y, x] for x, y, z in voxel)
        assert cluster.min() >= 0 and cluster.max() < len(keep) and np.all(np.diff(cluster) >= 0)
        assert [(int(c), tuple(int(t) for t in v)) for c, v in zip(cluster, voxel)] == model_proposals(w, keep, kf.camera2volume())
        cam_y = np.asarray(kf.camera2volume(), np.float64)[:3, 1, 0]
        for p in range(P):
            R = cands[p, :3, :3, 0].astype(np.float64)
            assert np.abs(R.T @ R - np.eye(3)).max() <= 8 * EPS and np.linalg.det(R) > 0
            to = got["centroid"][cluster[p]].astype(np.float64) - pos[p].astype(np.float64)
            dist = np.linalg.norm(to)
            assert dist > 0 and np.linalg.norm(np.cross(R[:, 2], to / dist)) <= 2 * EPS and R[:, 2] @ to > 0
            # the standoff, then per axis at most ORCH_SNAP voxels of snap and half a voxel from the standpoint to a centre (a whole one
            # here: room for the float32 roundings of the standpoint)
            assert dist <= ORCH_STANDOFF + (ORCH_SNAP + 1) * np.sqrt(3.0) * float(w["vs"])
            if abs(cam_y @ to) / dist <= 0.98:
                assert R[:, 1] @ cam_y > 0 and abs(R[:, 0] @ cam_y) <= 8 * EPS  # image-down leans towards the camera's, x is across it
        flags, clear2 = kf.reachable(cands, ORCH_RADIUS)
        assert flags.all() and P > int(before["reach"][0].sum())
        # explore_step: the model's pick over the same candidates, path_to's path
        cost = np.array([w["travel"][z, y, x] for x, y, z in voxel], np.uint16)
        assert (cost != tc.NONE).all()
        counts = kf.next_best_view(cands)[1]
        for bias_m, hits in ((0.5, None), (0.01, 0), (50.0, 0)):
            want = tc.next_view_by_travel(counts, cost, 80 * 60 // 4 if hits is None else hits, tc.travel_bias(bias_m, w["vs"]))
            step = kf.explore_step(ORCH_RADIUS, ORCH_VIEWS, ORCH_STANDOFF, ORCH_CELL, ORCH_MIN_SIZE, ORCH_SNAP, bias_m=bias_m, min_hits=hits)
            if want < 0:
                assert step is None
                continue
            assert step["index"] == want and np.array_equal(step["pose"], cands[want]) and step["cluster"] == cluster[want]
            assert np.array_equal(step["counts"], counts[want]) and step["travel_m"] == float(cost[want]) * float(w["vs"]) / 3.0
            points, voxels = kf.path_to(cands[want], ORCH_RADIUS)
            assert np.array_equal(step["path"][0], points) and np.array_equal(step["path"][1], voxels)
            assert tuple(int(t) for t in voxels[-1]) == tuple(int(t) for t in voxel[want]) and tuple(int(t) for t in voxels[0]) == tuple(int(t) for t in w["seed"][0])
        assert kf.explore_step(ORCH_RADIUS, ORCH_VIEWS, ORCH_STANDOFF, ORCH_CELL, ORCH_MIN_SIZE, ORCH_SNAP, min_hits=0) is not None
        assert kf.explore_step(ORCH_RADIUS, ORCH_VIEWS, ORCH_STANDOFF, ORCH_CELL, ORCH_MIN_SIZE, ORCH_SNAP, min_hits=10 ** 9) is None
        assert kf.explore_step(ORCH_RADIUS, ORCH_VIEWS, ORCH_STANDOFF, ORCH_CELL, 10 ** 9, ORCH_SNAP) is None   # no cluster that large: nothing proposed
        assert len(kf.propose_views(ORCH_RADIUS, 1, ORCH_STANDOFF, ORCH_CELL, ORCH_MIN_SIZE)[0]) <= len(keep)
        return dict(mask=m, P=P)

    a = check("after four frames:")
    # what was there before answers as before
    best, reach, travel, pick = kf.next_best_view(old), kf.reachable(old, ORCH_RADIUS), kf.travel(old, ORCH_RADIUS), kf.next_view_by_travel(old, ORCH_RADIUS)
    assert best[0] == before["best"][0] and np.array_equal(best[1], before["best"][1])
    assert all(np.array_equal(x, y) for x, y in zip(reach, before["reach"])) and all(np.array_equal(x, y) for x, y in zip(travel, before["travel"]))
    assert pick[0] == before["pick"][0] and np.array_equal(pick[1], before["pick"][1]) and np.array_equal(pick[2], before["pick"][2])
    for bad in (dict(cell_vox=12), dict(cell_vox=-8), dict(cell_vox=65536)):
        with pytest.raises(ValueError):
            kf.frontiers(**bad)
        with pytest.raises(ValueError):
            kf.propose_views(ORCH_RADIUS, **bad)
    for bad in (dict(radius_m=40.0), dict(radius_m=-1.0), dict(radius_m=ORCH_RADIUS, snap_vox=17), dict(radius_m=ORCH_RADIUS, start_snap_vox=17),
                dict(radius_m=ORCH_RADIUS, views_per_cluster=0), dict(radius_m=ORCH_RADIUS, standoff_m=-1.0), dict(radius_m=ORCH_RADIUS, standoff_m=float("nan"))):
        with pytest.raises(ValueError):
            kf.propose_views(**bad)
    assert kf.process_frame(dfr[4]) == 1
    b = check("after one more frame:")
    assert (a["mask"] != b["mask"]).any()
    kf.close()


def test_shard_mode_refuses(dev):
    """Two ranks as threads on one GPU: frontiers, propose_views and explore_step raise XsError on every rank and do nothing, and the pipeline
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
            for call in (lambda: shards[r].frontiers(), lambda: shards[r].propose_views(0.06), lambda: shards[r].explore_step(0.06)):
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
