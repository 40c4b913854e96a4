"""CPU-only: the host's side of travel cost and paths — the dijkstra model the kernels are held to against a scalar
brute force, its finite set against the flood's model, its symmetry, the path walk, the limit and bias derivations, the selection rule of
x-slam_amd/host/view_host.hpp against fractions.Fraction and under the sanitizers, the buffer sizes and the bindings."""
import importlib
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import reach_cases as rc
import travel_cases as tc


@pytest.fixture(scope="module")
def capi():
    return importlib.import_module("x-slam_amd.capi")


def random_domain(res, seed, p_free=0.78):
    """(domain, states, seeds): random FREE / OCCUPIED states, the domain is what a flood at r2 = 1 reaches from three passable seeds."""
    states = rc.random_states(res, seed, p=(0.0, p_free, 1.0 - p_free))
    field = rc.clearance(states, 1, 0)
    free = np.argwhere(rc.passable_of(states, field, 1))
    pick = np.random.default_rng(seed).choice(len(free), 3, replace=False)
    seeds = [tuple(int(v) for v in free[i][::-1]) for i in pick]
    return rc.reached(states, field, 1, seeds), states, seeds


@pytest.mark.parametrize("res", [(7, 6, 5), (5, 4, 9)])
@pytest.mark.parametrize("limit", [0, 10, 65534])
def test_model_equals_brute_force(res, limit):
    """scipy's dijkstra over the explicit graph against a heap with per-voxel neighbour tests; seeds outside the volume and outside the
    domain contribute nothing; limit 0 leaves the seeds only."""
    domain, states, seeds = random_domain(res, seed=4 + res[0])
    blocked = tuple(int(v) for v in np.argwhere(~domain)[0][::-1])
    for ss in ([seeds[0]], seeds, seeds + [blocked, (-1, 0, 0), (res[0], 1, 1)], [blocked]):
        got, want = tc.model(domain, ss, limit), tc.brute(domain, ss, limit)
        assert got.dtype == np.uint16 and np.array_equal(got, want), (ss, np.argwhere(got != want)[:5])
        inside = [s for s in ss if s != blocked and 0 <= s[0] < res[0]]
        assert all(got[z, y, x] == 0 for x, y, z in inside)
        if limit == 0:
            assert (got != tc.NONE).sum() == len(set(inside))
        else:
            assert not inside or (got != tc.NONE).sum() > len(set(inside))
        assert got[got != tc.NONE].max(initial=0) <= limit
    assert np.all(tc.model(domain, [blocked], limit) == tc.NONE)


@pytest.mark.parametrize("res", [(20, 18, 13), (19, 18, 13)])
def test_finite_set_is_the_reached_set_and_diagonals_matter(res):
    """With the limit out of the way the voxels with a finite cost are exactly the flood's reached set (an allowed diagonal move implies a
    6-connected detour); most voxels use a diagonal move (their cost is below three times the 6-connected distance), and without the
    corner rule values change."""
    domain, states, seeds = random_domain(res, seed=3)
    one = [seeds[0]]
    field = rc.clearance(states, 1, 0)
    reached = rc.reached(states, field, 1, one)
    free = rc.passable_of(states, field, 1)
    got = tc.model(free, one)                                                    # over all passable voxels: the model finds the component itself
    assert np.array_equal(got != tc.NONE, reached) and reached.sum() > 1000
    faces = tc.model(free, one).astype(np.int64)
    six = np.full(free.shape, 1 << 30, np.int64)
    six[one[0][2], one[0][1], one[0][0]] = 0
    while True:                                                                   # 3 x the face-connected distance by plain relaxation
        nxt = six.copy()
        for o in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
            cand = np.where(tc.shifted(free, o), np.roll(six, (-o[2], -o[1], -o[0]), (0, 1, 2)) + 3, 1 << 30)
            nxt = np.where(free & (cand < nxt), cand, nxt)
        if np.array_equal(nxt, six):
            break
        six = nxt
    assert np.array_equal(six < (1 << 30), reached) and (faces[reached] <= six[reached]).all()
    assert (faces[reached] < six[reached]).mean() > 0.5
    cut = tc.model(free, one, corner_rule=False)
    assert np.array_equal(cut != tc.NONE, reached) or (cut != tc.NONE).sum() > reached.sum()
    assert (cut[reached] != got[reached]).mean() > 0.3 and (cut[reached] <= got[reached]).all()


def test_field_is_symmetric_between_two_seeds():
    """The move rule is symmetric in v and v + o, so the cost from a to b is the cost from b to a."""
    domain, _, seeds = random_domain((20, 18, 13), seed=3)
    pts = [tuple(int(v) for v in p[::-1]) for p in np.argwhere(domain)[:: max(1, int(domain.sum()) // 12)]]
    fields = {p: tc.model(domain, [p]) for p in pts}
    for a in pts:
        for b in pts:
            assert fields[a][b[2], b[1], b[0]] == fields[b][a[2], a[1], a[0]]
    assert len(pts) >= 10 and fields[pts[0]][pts[-1][2], pts[-1][1], pts[-1][0]] not in (0, tc.NONE)


def test_path_walk():
    """Every step of a walked path is an allowed move, the weights add up to travel[target], the path ends on a seed, and among several
    moves that explain a value the lowest index k is taken."""
    domain, _, seeds = random_domain((20, 18, 13), seed=3)
    travel = tc.model(domain, seeds)
    targets = [tuple(int(v) for v in p[::-1]) for p in np.argwhere(domain)[::97]]
    ties = 0
    for t in targets:
        path = tc.walk(travel, domain, t)
        assert path[0] == t and travel[path[-1][2], path[-1][1], path[-1][0]] == 0 and path[-1] in seeds
        total = 0
        for a, b in zip(path[:-1], path[1:]):
            o = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
            assert max(abs(c) for c in o) == 1 and tc.move_allowed(domain, a, o)
            total += tc.cost_of(o)
            k = tc.MOVES.index(o)
            explains = [j for j, m in enumerate(tc.MOVES) if j != 13 and tc.move_allowed(domain, a, m)
                        and int(travel[a[2] + m[2], a[1] + m[1], a[0] + m[0]]) + tc.cost_of(m) == int(travel[a[2], a[1], a[0]])]
            assert k == min(explains)
            ties += len(explains) > 1
        assert total == int(travel[t[2], t[1], t[0]])
    assert ties >= 10 and len(targets) >= 20
    assert tc.walk(travel, domain, seeds[0]) == [seeds[0]]
    blocked = tuple(int(v) for v in np.argwhere(~domain)[0][::-1])
    assert tc.walk(travel, domain, blocked) == [] and tc.walk(travel, domain, (-1, 2, 2)) == [] and tc.walk(travel, domain, (2, 2, 13)) == []
    # an open box: from (2, 2, 2) to the seed (0, 0, 0) the corner move k = 0 explains the value and comes first
    box = np.ones((4, 4, 4), bool)
    t = tc.model(box, [(0, 0, 0)])
    assert t[2, 2, 2] == 10 and tc.walk(t, box, (2, 2, 2)) == [(2, 2, 2), (1, 1, 1), (0, 0, 0)]
    assert t[0, 1, 2] == 7 and tc.walk(t, box, (2, 1, 0)) == [(2, 1, 0), (1, 0, 0), (0, 0, 0)]   # k = 9 (-1, -1, 0) before k = 12 (-1, 0, 0)


def test_limit_and_bias_derivations():
    """travel_limit and travel_bias in float32, on and beside integer multiples of a binary voxel size."""
    up, down = (lambda v: np.nextafter(np.float32(v), np.float32(1e9))), (lambda v: np.nextafter(np.float32(v), np.float32(-1e9)))
    assert [tc.travel_limit(m, 0.125) for m in (0.0, -1.0, np.inf, np.nan)] == [65534] * 4
    assert (tc.travel_limit(1.0, 0.125), tc.travel_limit(down(1.0), 0.125), tc.travel_limit(up(1.0), 0.125)) == (24, 23, 24)
    assert (tc.travel_limit(0.125, 0.125), tc.travel_limit(0.04, 0.125), tc.travel_limit(0.05, 0.125)) == (3, 0, 1)
    assert (tc.travel_limit(2730.0, 0.125), tc.travel_limit(2730.6, 0.125), tc.travel_limit(1e30, 0.125), tc.travel_limit(3e38, 0.125)) == (65520, 65534, 65534, 65534)
    for k in range(1, 21845, 7):
        assert tc.travel_limit(0.25 * k, 0.25) == 3 * k
    assert [tc.travel_bias(b, 0.125) for b in (0.0, 0.01, 0.125, 0.5, -3.0)] == [1, 1, 3, 12, 1]
    assert (tc.travel_bias(up(0.5), 0.125), tc.travel_bias(down(0.5), 0.125)) == (13, 12)
    assert tc.travel_limit(1.0, 0.13) == 23 and tc.travel_limit(1.0, 3.0 / 64.0) == 64 and tc.travel_bias(0.5, 0.12) == 13


def test_selection_rule_against_fractions():
    """unknown / (travel + bias3) compared exactly: random tables against fractions.Fraction (ties to the lower index), and a pair that
    float32 would order wrongly."""
    rng = np.random.default_rng(11)
    for trial in range(200):
        P = int(rng.integers(1, 12))
        out = np.zeros((P, 4), np.uint32)
        out[:, 0] = rng.integers(0, 40, P) if trial % 2 else rng.integers(0, 2 ** 32, P, dtype=np.uint64)
        out[:, 2] = rng.integers(0, 20, P)
        travel = rng.choice(np.array([0, 3, 4, 5, 7, 30, 65534, tc.NONE], np.uint16), P)
        bias, hits = int(rng.choice([1, 3, 13, 1 << 30])), int(rng.integers(0, 20))
        ok = [p for p in range(P) if travel[p] != tc.NONE and out[p, 2] >= hits]
        want = -1
        for p in ok:
            if want < 0 or Fraction(int(out[p, 0]), int(travel[p]) + bias) > Fraction(int(out[want, 0]), int(travel[want]) + bias):
                want = p
        assert tc.next_view_by_travel(out, travel, hits, bias) == want
    big = np.array([[4000000000, 0, 1, 0], [2000000001, 0, 1, 0]], np.uint32)
    assert tc.next_view_by_travel(big, np.array([1, 0], np.uint16), 1, 1) == 1
    assert np.float32(4000000000) / np.float32(2) == np.float32(2000000001) / np.float32(1)   # float32 sees a tie and would keep 0
    assert tc.next_view_by_travel(big, np.array([tc.NONE, tc.NONE], np.uint16), 0, 1) == -1


def test_travel_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/view_host.hpp's travel_limit, travel_bias and next_view_by_travel compiled with -fsanitize=address,undefined
    -fno-sanitize-recover and run (tests/cxx/travel_selftest.cpp); the Python twins of travel_cases.py give the same answers on its tables."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "travel_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(root, "x-slam_amd", "host"), os.path.join(root, "tests", "cxx", "travel_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    a = np.array([[100, 5, 10, 1], [900, 0, 0, 7], [300, 9, 10, 2], [300, 1, 50, 3], [50, 2, 400, 0], [300, 4, 9, 4]], np.uint32)
    t1 = np.array([3, 65535, 30, 12, 0, 27], np.uint16)
    assert [tc.next_view_by_travel(a, t1, h, b) for h, b in ((0, 3), (51, 3), (0, 300), (0, 1), (401, 3))] == [3, 4, 3, 4, -1]
    assert tc.next_view_by_travel(a, np.array([0, 0, 10, 10, 0, 10], np.uint16), 9, 3) == 0


def test_sizes(capi):
    """Two bytes per voxel of field, a small workspace of control words; 0 for bad resolutions."""
    for r in ((1, 1, 1), (3, 3, 3), (19, 18, 13), (300, 4, 5), (64, 64, 64), (512, 512, 512)):
        assert capi.travel_bytes(r) == 2 * r[0] * r[1] * r[2]
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (4, 70000, 4), (4, 4, 70000)):
        assert capi.travel_bytes(bad) == 0, bad
    assert 32 <= capi.travel_workspace_bytes() <= 4096 and capi.travel_workspace_bytes() % 4 == 0


def test_bindings_exist(capi):
    """The entry points of every layer: the library's symbols with their ctypes signatures, the orchestrator's C ABI and the methods of
    KinectFusion (ShardedKinectFusion inherits them; in shard mode they raise XsError — the GPU suite)."""
    pl = importlib.import_module("x-slam_amd.pipeline")
    sh = importlib.import_module("x-slam_amd.sharded")
    for n in ("xs_travel_bytes", "xs_travel_workspace_bytes", "xs_travel_build", "xs_travel_query", "xs_travel_path"):
        assert n in capi._SIGS and hasattr(capi._lib, n), n
    for n in ("xs_kf_travel", "xs_kf_path_to", "xs_kf_next_view_by_travel"):
        assert n in pl._SIGS and hasattr(pl._lib, n), n
    assert (capi.TRAVEL_NONE, capi.TRAVEL_MAX, capi.TRAVEL_MAX_TARGETS) == (65535, 65534, 64) and capi.abi_version() == 3
    for cls in (pl.KinectFusion, sh.ShardedKinectFusion):
        assert callable(cls.travel) and callable(cls.path_to) and callable(cls.next_view_by_travel)
    for f in ("travel_bytes", "travel_workspace_bytes", "travel_build", "travel_query", "travel_path"):
        assert callable(getattr(capi, f))
