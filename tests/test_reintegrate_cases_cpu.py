"""CPU: the model of signed re-integration (tests/reintegrate_cases.py) on synthetic observations — the rules of include/xslam_amd.h one by
one, and the derived rounding bound against the exact mean — and the binding's constants.  tests/test_reintegrate_gpu.py holds the kernel to
this model."""
import importlib
import itertools

import numpy as np

import reintegrate_cases as rc


def observations(k, n=4096, seed=3):
    rng = np.random.default_rng(seed)
    obs = []
    for _ in range(k):
        tv = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        tv[rng.random(n) < 0.3] = np.float32(1.0)          # free space in front of a surface
        tv[rng.random(n) < 0.05] = np.float32(-1.0)
        tg = (rng.uniform(-1.0, 1.0, n) * 1e-6).astype(np.float32)
        tg[tv == 1.0] = np.float32(0.0)
        obs.append((tv, tg))
    return obs


def test_binding_constants():
    capi = importlib.import_module("x-slam_amd.capi")
    assert capi.REINTEGRATE_MAX_OPS == 8 and capi.abi_version() == 3
    assert capi.REINTEGRATE_NO_CULL == 1
    import ctypes
    assert ctypes.sizeof(capi.ReintegrateOp) == 8 + 8 + 24 * 4     # sign and its padding, the image pointer, the pose


def test_addition_is_the_running_mean_with_the_weight_clamp():
    n = 1000
    rng = np.random.default_rng(1)
    (tv, tg), = observations(1, n)
    v = rng.uniform(-1, 1, n).astype(np.float32)
    g = (rng.uniform(-1, 1, n) * 1e-6).astype(np.float32)
    w = rng.integers(0, rc.MAX_WEIGHT + 1, n).astype(np.int32)
    w[:50] = rc.MAX_WEIGHT
    seen = rng.random(n) < 0.7
    nv, nw, ng, counts = rc.apply((v, w, g), [(1, seen, tv, tg)])
    wf = w.astype(np.float32)
    want_v = ((v * wf + tv) / (w + 1).astype(np.float32)).astype(np.float32)
    want_g = ((g * wf + tg) / (w + 1).astype(np.float32)).astype(np.float32)
    assert rc.same_words(nv[seen], want_v[seen]) and rc.same_words(ng[seen], want_g[seen])
    assert np.array_equal(nw[seen], np.minimum(w[seen] + 1, rc.MAX_WEIGHT)) and (nw[:50][seen[:50]] == rc.MAX_WEIGHT).all()
    assert rc.same_words(nv[~seen], v[~seen]) and rc.same_words(ng[~seen], g[~seen]) and np.array_equal(nw[~seen], w[~seen])
    assert counts == [0, int(seen.sum()), 0, 0]


def test_add_then_remove_on_an_empty_voxel_is_the_init_state():
    (tv, tg), = observations(1, 512)
    seen = np.ones(512, bool)
    v, w, g, counts = rc.apply(rc.empty((512, 1, 1)), [(1, seen.reshape(1, 1, 512), tv.reshape(1, 1, 512), tg.reshape(1, 1, 512)),
                                                       (-1, seen.reshape(1, 1, 512), tv.reshape(1, 1, 512), tg.reshape(1, 1, 512))])
    zero = np.zeros((1, 1, 512), np.float32)
    assert rc.same_words(v, zero) and rc.same_words(g, zero) and not w.any()       # +0, as xs_init_volume leaves
    assert counts == [512, 512, 512, 0]


def test_removing_one_of_k_stays_within_the_bound_of_the_mean_of_the_others():
    n = 4096
    assert rc.bound_u(6, 1) == 34.0 and rc.bound_u(1, 0) == 0.0 and rc.bound_u(2, 0) == 3.0 and rc.bound_u(6, 2) == 72.0
    seen = np.ones(n, bool)
    worst = 0.0
    for k in range(2, 7):
        obs = observations(k, n, seed=10 + k)
        Mg = np.max([np.abs(tg) for _, tg in obs], axis=0)
        for j in range(k):
            ops = [(1, seen, tv, tg) for tv, tg in obs] + [(-1, seen) + obs[j]]
            v, w, g, counts = rc.apply((np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)), ops)
            v64, w64, g64, _ = rc.apply((np.zeros(n), np.zeros(n, np.int32), np.zeros(n)), ops, dtype=np.float64)
            mv, mg = rc.exact_mean(obs, [i for i in range(k) if i != j])
            assert (w == k - 1).all() and np.array_equal(w, w64) and counts == [n, k * n, 0, 0]
            ev, eg = np.abs(v.astype(np.float64) - mv), np.abs(g.astype(np.float64) - mg)
            assert ev.max() <= rc.bound(k, 1), (k, j, ev.max() / rc.U)
            assert (eg <= rc.bound(k, 1, 1.0) * Mg).all(), (k, j)
            assert np.abs(v64 - mv).max() <= 1e-12          # the twin is the exact mean to float64 rounding
            worst = max(worst, ev.max() / rc.U)
    assert worst > 0.5      # the bound is about rounding that does occur


def test_removal_without_weight_is_orphaned():
    n = 64
    (tv, tg), = observations(1, n)
    v = np.linspace(-1, 1, n).astype(np.float32)
    g = np.full(n, 3e-7, np.float32)
    w = np.zeros(n, np.int32)
    nv, nw, ng, counts = rc.apply((v, w, g), [(-1, np.ones(n, bool), tv, tg)])
    assert rc.same_words(nv, v) and rc.same_words(ng, g) and not nw.any() and counts == [0, 0, 0, n]


def test_the_clamp_acts_on_the_real_part_only():
    # weight 2, value 1, grad 3: removing t = (-1, -5) gives (2 + 1, 6 + 5) / 1 = (3, 11): the real part is clamped, the imaginary part kept
    one = np.ones(2, np.float32)
    v, w, g, counts = rc.apply((one * [1.0, -1.0], np.full(2, 2, np.int32), one * [3.0, -3.0]),
                               [(-1, np.ones(2, bool), one * [-1.0, 1.0], one * [-5.0, 5.0])])
    assert v.tolist() == [1.0, -1.0] and g.tolist() == [11.0, -11.0] and w.tolist() == [1, 1] and counts == [2, 0, 0, 0]
    v64, _, g64, _ = rc.apply((np.array([1.0, -1.0]), np.full(2, 2, np.int32), np.array([3.0, -3.0])),
                              [(-1, np.ones(2, bool), one * [-1.0, 1.0], one * [-5.0, 5.0])], dtype=np.float64)
    assert v64.tolist() == [1.0, -1.0] and g64.tolist() == [11.0, -11.0]


def test_ops_apply_in_list_order():
    # a voxel emptied by op 1 is refilled by op 2; the other order averages first and removes then
    a = (np.float32(0.25), np.float32(1e-7))
    b = (np.float32(-0.5), np.float32(-2e-7))
    state = (np.array([a[0]], np.float32), np.array([1], np.int32), np.array([a[1]], np.float32))
    seen = np.ones(1, bool)
    v, w, g, counts = rc.apply(state, [(-1, seen, np.array([a[0]]), np.array([a[1]])), (1, seen, np.array([b[0]]), np.array([b[1]]))])
    assert v[0] == b[0] and g[0] == b[1] and w[0] == 1 and counts == [1, 1, 1, 0]
    v, w, g, counts = rc.apply(state, [(1, seen, np.array([b[0]]), np.array([b[1]])), (-1, seen, np.array([a[0]]), np.array([a[1]]))])
    assert v[0] == b[0] and w[0] == 1 and counts == [1, 1, 0, 0]
    assert abs(float(g[0]) - float(b[1])) <= rc.bound(2, 1, 2e-7)


def test_counts_over_mixed_masks():
    n = 200
    rng = np.random.default_rng(5)
    obs = observations(3, n)
    w = rng.integers(0, 4, n).astype(np.int32)
    v = rng.uniform(-1, 1, n).astype(np.float32)
    g = np.zeros(n, np.float32)
    masks = [rng.random(n) < 0.6 for _ in range(3)]
    signs = (-1, -1, 1)
    _, nw, _, counts = rc.apply((v, w, g), [(s, m) + o for s, m, o in zip(signs, masks, obs)])
    ww = w.astype(np.int64).copy()
    want = [0, 0, 0, 0]
    for s, m in zip(signs, masks):
        for i in np.flatnonzero(m):
            if s > 0:
                ww[i] = min(ww[i] + 1, rc.MAX_WEIGHT); want[1] += 1
            elif ww[i] >= 2:
                ww[i] -= 1; want[0] += 1
            elif ww[i] == 1:
                ww[i] = 0; want[0] += 1; want[2] += 1
            else:
                want[3] += 1
    assert counts == want and np.array_equal(nw, ww) and all(c > 0 for c in want)


def test_scenes_are_inside_the_valid_depth_range():
    for shape, size in itertools.product(rc.shapes(), (0, 1)):
        s = rc.scene(shape, size)
        for which in (0, 1):
            mm = rc.depth_image(s["rows"], s["cols"], which)
            valid = mm[mm > 0]
            assert valid.min() >= 200 and valid.max() <= 5000 and 0.03 < (mm == 0).mean() < 0.2
        assert set(rc.poses(shape, s["voxel_size"])) == {"front", "inside", "oblique", "seeded", "away", "back"}
    assert all(len(ops) <= 8 for ops in rc.OP_LISTS.values()) and len(rc.OP_LISTS["eight"]) == 8
