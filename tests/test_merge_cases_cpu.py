"""CPU-only: the model the volume merge is held to (tests/merge_cases.py) against its float64 twin and against the consequences of the
contract (an identity into an empty volume is a copy, a whole-voxel shift a slice, the 24 axis permutations exact), the host algebra of
x-slam_amd/host/merge_host.hpp through the exported functions and under the sanitizers, the buffer size and the bindings."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import merge_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in mc.SHAPES if s[0] != (33, 1028, 3)] + [((33, 70, 3), (9, 10, 130))]


@pytest.fixture(scope="module")
def pl():
    return importlib.import_module("x-slam_amd.pipeline")


@pytest.mark.parametrize("dshape,sshape", mc.SHAPES)
def test_model_agrees_with_its_float64_twin(dshape, sshape):
    """Every map, both min_weights, into the populated and the empty destination: value and grad within MODEL_BOUND_U u M of the twin,
    weights and `written` equal; and the cases are what the module says they are (skipped voxels, partial neighbourhoods, capped sums,
    2-, 4- and 8-corner voxels)."""
    dst, src = mc.volumes(dshape, sshape)
    bound = mc.model_bound(dst, src)
    corners = set()
    capped = partial = 0
    for name, m in mc.maps(dshape, sshape).items():
        for mw in mc.MIN_WEIGHTS:
            for populated in (True, False):
                d = dst if populated else mc.empty_volume(dshape)
                v32, w32, g32, n32 = mc.expected(dshape, sshape, name, mw, populated)
                v64, w64, g64, n64, det = mc.merge(d, src, m, mw, dtype=np.float64, details=True)
                assert v32.dtype == np.float32 and g32.dtype == np.float32 and v64.dtype == np.float64
                assert n32 == n64 and np.array_equal(w32, w64)
                assert np.abs(v32.astype(np.float64) - v64).max(initial=0) <= bound, (name, mw, populated)
                assert np.abs(g32.astype(np.float64) - g64).max(initial=0) <= bound, (name, mw, populated)
                assert not np.isnan(v32).any() and not np.isnan(g32).any()
                ok = det["ok"]
                corners |= set(np.unique((1 << (det["need"][0].astype(int) + det["need"][1] + det["need"][2]))[ok]).tolist())
                capped += int((w32[ok] == mc.MAX_WEIGHT).sum())
                partial += int((det["inside"] & ~ok).sum())
                if name == "miss":
                    assert n32 == 0 and mc.same_bits(v32, d[0]) and np.array_equal(w32, d[1])
    if min(dshape) > 2:
        assert corners == {1, 2, 4, 8} and capped > 0 and partial > 0, (corners, capped, partial)


@pytest.mark.parametrize("dshape,sshape", SMALL)
def test_identity_into_an_empty_volume_is_a_copy(dshape, sshape):
    """Bit for bit where the source carries min_weight, far faces included; -0 stays -0."""
    _, src = mc.volumes(sshape, sshape)
    for mw in mc.MIN_WEIGHTS:
        v, w, g, n = mc.merge(mc.empty_volume(sshape), src, mc.xform(), mw)
        keep = src[1] >= mw
        assert n == keep.sum()
        assert mc.same_bits(v, np.where(keep, src[0], np.float32(0))) and mc.same_bits(g, np.where(keep, src[2], np.float32(0)))
        assert np.array_equal(w, np.where(keep, src[1], 0))
    assert (np.signbit(src[0]) & (src[0] == 0)).any()


@pytest.mark.parametrize("shift", [(3, -2, 1), (-1, 0, 2), (0, 1, 0)])
def test_a_whole_voxel_shift_is_a_slice(shift):
    """g = d + shift: destination voxel d takes source voxel d + shift where that exists, the rest is untouched."""
    dshape, sshape = (9, 8, 7), (11, 6, 9)
    dst, src = mc.volumes(dshape, sshape)
    v, w, g, n = mc.merge(mc.empty_volume(dshape), src, mc.xform(offset=shift), 1)
    want = [np.zeros_like(a) for a in mc.empty_volume(dshape)]
    count = 0
    for z in range(dshape[2]):
        for y in range(dshape[1]):
            for x in range(dshape[0]):
                s = (x + shift[0], y + shift[1], z + shift[2])
                if all(0 <= s[a] < sshape[a] for a in range(3)) and src[1][s[2], s[1], s[0]] >= 1:
                    for k in range(3):
                        want[k][z, y, x] = src[k][s[2], s[1], s[0]]
                    count += 1
    assert n == count > 0 and mc.same_bits(v, want[0]) and np.array_equal(w, want[1]) and mc.same_bits(g, want[2])
    # into the populated destination the voxels outside the overlap keep their bits
    v, w, g, n2 = mc.merge(dst, src, mc.xform(offset=shift), 1)
    out = want[1] == 0
    assert n2 == n and mc.same_bits(v[out], dst[0][out]) and np.array_equal(w[out], dst[1][out]) and mc.same_bits(g[out], dst[2][out])


def test_the_24_axis_permutations_are_exact():
    """A cube of side 6 under each proper rotation of the cube into an empty cube: the numpy transpose and flip of the source, bit for bit."""
    shape = (6, 6, 6)
    _, src = mc.volumes(shape, shape)
    P = mc.signed_permutations()
    assert len(P) == 24
    seen = set()
    for Pm in P:
        m = mc.permutation_map(Pm, shape)
        v, w, g, n = mc.merge(mc.empty_volume(shape), src, m, 1)
        # source index a = d[p(a)], counted down from 5 on a flipped axis: an integer gather, no arithmetic on the values
        d = np.meshgrid(np.arange(6), np.arange(6), np.arange(6), indexing="ij")[::-1]          # d[0] = x, d[1] = y, d[2] = z, each [z, y, x]
        s = []
        for a in range(3):
            p = int(np.flatnonzero(Pm[a])[0])
            s.append(5 - d[p] if Pm[a].sum() < 0 else d[p])
        want = [arr[s[2], s[1], s[0]] for arr in src]
        keep = want[1] >= 1
        assert n == keep.sum()
        assert mc.same_bits(v, np.where(keep, want[0], np.float32(0))) and np.array_equal(w, np.where(keep, want[1], 0))
        assert mc.same_bits(g, np.where(keep, want[2], np.float32(0)))
        seen.add(v.tobytes())
    assert len(seen) == 24


def test_merge_affine_to_the_last_bit(pl):
    """xs_host_merge_affine against the float64 numpy restatement on the three voxel sizes and on unequal sizes with ratios 2 and 0.5, for
    the identity, whole-voxel shifts and random rigid transforms; and its refusals."""
    capi = importlib.import_module("x-slam_amd.capi")
    rng = np.random.default_rng(41)
    Ts = [np.eye(4)]
    for _ in range(40):
        T = np.eye(4)
        T[:3, :3] = mc.rotation(rng.normal(size=3), rng.uniform(-3, 3))
        T[:3, 3] = rng.uniform(-5, 5, 3)
        Ts.append(T)
    n = 0
    for vs in mc.VOXEL_SIZES:
        vs = float(np.float32(vs))
        shift = np.eye(4)
        shift[:3, 3] = np.array([3, -2, 5]) * vs
        for vd, vsrc in ((vs, vs), (2 * vs, vs), (0.5 * vs, vs), (vs, 2 * vs)):
            for T in Ts + [shift]:
                got, want = pl.merge_affine(T, vd, vsrc), mc.affine64(T, vd, vsrc)
                assert got.dtype == np.float32 and mc.same_bits(got, want), (vs, vd, vsrc)
                assert mc.same_bits(capi.merge_affine(T, vd, vsrc), want)
                n += 1
        m = pl.merge_affine(shift, vs, vs)
        assert np.array_equal(m[:9].reshape(3, 3), np.eye(3, dtype=np.float32)) and np.abs(m[9:] - np.array([3, -2, 5], np.float32)).max() <= 8 * mc.U * 5
    assert n == 3 * 4 * 42
    assert np.array_equal(pl.merge_affine(np.eye(4), 0.25, 0.125), mc.xform(2 * np.eye(3), (0.5, 0.5, 0.5)))
    # a complex pose [4, 4, 2]: the real parts
    c = np.zeros((4, 4, 2))
    c[..., 0], c[..., 1] = Ts[3], 1e-7
    assert mc.same_bits(pl.merge_affine(c, 0.1, 0.05), mc.affine64(Ts[3], 0.1, 0.05))
    for bad in (np.full((4, 4), np.nan), np.diag([1, 1, np.inf, 1])):
        with pytest.raises(ValueError):
            pl.merge_affine(bad, 0.1, 0.1)
    for vd, vsrc in ((0.0, 0.1), (0.1, 0.0), (-0.1, 0.1), (np.inf, 0.1)):
        with pytest.raises(ValueError):
            pl.merge_affine(np.eye(4), vd, vsrc)


def test_map_transform_round_trips(pl):
    """T = c2v_other c2v_this^-1: T c2v_this = c2v_other to float64 accuracy, map_transform(a, a) is the identity, the two directions are
    inverses; the imaginary parts of complex poses are ignored."""
    rng = np.random.default_rng(43)
    for _ in range(50):
        A, B = np.eye(4), np.eye(4)
        for M in (A, B):
            M[:3, :3] = mc.rotation(rng.normal(size=3), rng.uniform(-3, 3))
            M[:3, 3] = rng.uniform(-5, 5, 3)
        T = pl.map_transform(A, B)
        assert T.dtype == np.float64 and np.abs(T @ A - B).max() < 1e-13 and np.array_equal(T[3], [0, 0, 0, 1])
        assert np.abs(pl.map_transform(A, A) - np.eye(4)).max() < 1e-14
        assert np.abs(T @ pl.map_transform(B, A) - np.eye(4)).max() < 1e-13
        Ac = np.stack([A, rng.normal(size=(4, 4))], axis=-1)
        assert np.array_equal(pl.map_transform(Ac, B), T)


def test_cull_box_contains_every_voxels_source_box(pl):
    """merge_tile_box of merge_host.hpp (the text the kernel compiles), through the exported function: for random affine maps and tiles, every
    voxel of the tile that the model lets through reads corners inside the box, and a tile reported as a miss holds no such voxel."""
    rng = np.random.default_rng(47)
    hits = misses = 0
    for it in range(400):
        S = tuple(int(s) for s in rng.integers(1, 70, 3))
        lo = np.array([64, 4, 4]) * rng.integers(0, 6, 3)
        hi = lo + rng.integers(0, [64, 4, 4])
        if it % 3 == 0:        # a rotation with a scale that takes the tile's middle to a point in or near the source
            R = mc.rotation(rng.normal(size=3), rng.uniform(-3, 3)) * rng.uniform(0.3, 2.5)
            m = mc.xform(R, rng.uniform(-0.3, 1.3, 3) * np.array(S) - R @ (0.5 * (lo + hi)))
        elif it % 3 == 1:      # whole and half voxel shifts around the tile's own origin: indices exactly on faces
            m = mc.xform(offset=rng.integers(-20, 20, 3) * 0.5 - lo)
        else:                  # anything
            m = rng.uniform(-3, 3, 12).astype(np.float32)
        box = pl.merge_tile_box(m, lo, hi, S)
        # the model's cells on a destination just large enough to hold the tile
        inside, b, f, need = mc.cells(m, tuple(int(h) + 1 for h in hi), S)
        tile = np.zeros(inside.shape, bool)
        tile[lo[2]:, lo[1]:, lo[0]:] = True
        sel = inside & tile
        if box is None:
            misses += 1
            assert not sel.any()
            continue
        hits += 1
        blo, bhi = box
        assert all(0 <= blo[a] <= bhi[a] <= S[a] - 1 for a in range(3))
        for a in range(3):
            if sel.any():
                assert blo[a] <= b[a][sel].min() and (b[a] + need[a])[sel].max() <= bhi[a]
    assert hits > 50 and misses > 50


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/merge_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/merge_selftest.cpp)."""
    exe = str(tmp_path / "merge_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "x-slam_amd", "host"), os.path.join(ROOT, "tests", "cxx", "merge_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_sizes_and_bindings(pl):
    """One bit per brick of 4 x 4 x 4 source voxels behind a header, 0 for an unusable resolution; the entry points of every layer."""
    capi = importlib.import_module("x-slam_amd.capi")
    sh = importlib.import_module("x-slam_amd.sharded")
    for s in ((1, 1, 1), (9, 10, 130), (64, 64, 64), (512, 512, 512), (1024, 1024, 513)):
        bricks = -(-s[0] // 4) * -(-s[1] // 4) * -(-s[2] // 4)
        n = capi.tsdf_merge_workspace_bytes((8, 8, 8), s)
        assert n % 256 == 0 and 256 + bricks / 8 <= n <= 256 + bricks / 8 + 512, (s, n)
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (4, 300000, 4)):
        assert capi.tsdf_merge_workspace_bytes((8, 8, 8), bad) == 0 and capi.tsdf_merge_workspace_bytes(bad, (8, 8, 8)) == 0
    for n in ("xs_tsdf_merge", "xs_tsdf_merge_workspace_bytes"):
        assert n in capi._SIGS and hasattr(capi._lib, n), n
    for n in ("xs_kf_merge_volume", "xs_kf_merge_map", "xs_kf_merge_checkpoint", "xs_host_merge_affine", "xs_host_map_transform", "xs_host_merge_tile_box"):
        assert n in pl._SIGS and hasattr(pl._lib, n), n
    assert capi.MERGE_NO_CULL == 1 and capi.abi_version() == 3
    for cls in (pl.KinectFusion, sh.ShardedKinectFusion):
        assert callable(cls.merge_map) and callable(cls.merge_checkpoint)
    assert callable(pl.map_transform) and callable(capi.tsdf_merge) and callable(capi.map_transform)
    assert len(mc.maps(*mc.SHAPES[3])) >= 16 and len(mc.pitch_pairs(*mc.SHAPES[3])) == 16
