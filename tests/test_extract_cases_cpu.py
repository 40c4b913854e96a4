"""CPU: the float32 model of surface export (tests/extract_cases.py) against the oracle's restatement, bit for bit; the model's order;
the model against its float64 twin within the derived bounds; and the conditions the cases have to meet for the GPU tests
(tests/test_extract_ragged_gpu.py) to mean something.  No GPU."""
import numpy as np
import pytest

import extract_cases as ec

ALL_SHAPES = ec.SHAPES + list(ec.SCAN_SHAPES)


def lexsorted(p):
    return p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]


def flat(value, shape):
    return np.ascontiguousarray(value).reshape(-1, shape[0])


def cases_of(shape):
    c = [ec.random_case(shape)]
    if shape in ec.SCAN_SHAPES:
        c.append(ec.sparse_case(shape))
    if shape == (2, 2, 2):
        c.append(ec.empty_case(shape))
    return c


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_model_equals_oracle(oracle, shape):
    for c in cases_of(shape):
        v2 = flat(c["value"], shape)
        op, ofound = oracle.extract_points(v2, list(shape), c["vs"])
        assert ofound == c["found"] == len(op)
        assert ec.same_bits(lexsorted(op), lexsorted(c["points"]))
        # the oracle appends in (z, y, x, direction) order: the model's points, put in that order by the voxel and direction the
        # model ascribes them to, are the oracle's array as it stands
        X, Y, Z = shape
        key = ((c["z"] * Y + c["y"]) * X + c["x"]) * 3 + c["d"]
        assert len(np.unique(key)) == len(key)
        assert ec.same_bits(c["points"][np.argsort(key)], op)
        assert ec.same_normals(oracle.extract_normals(v2, list(shape), c["vs"], c["points"]), c["normals"])
        assert ec.same_normals(oracle.extract_normals(v2, list(shape), c["vs"], c["general"]), c["general_normals"])


def test_model_equals_oracle_on_plane_ranges(oracle):
    shape = ec.SLAB_SHAPE
    X, Y, Z = shape
    c = ec.random_case(shape)
    for zs0, z0, z1 in ((0, 0, 3), (0, 3, 4), (0, 4, 10), (2, 3, 4), (2, 4, 10), (4, 4, 10)):
        stored = c["value"][zs0:]
        op, ofound = oracle.extract_points(flat(stored, shape), list(shape), c["vs"], z0=z0, z1=z1, zs0=zs0)
        mp, mfound = ec.points(stored, shape, c["vs"], zs0, z0, z1)
        assert ofound == mfound > 0 and ec.same_bits(lexsorted(op), lexsorted(mp))
        whole = (c["z"] >= z0) & (c["z"] < z1)
        assert ec.same_bits(mp, c["points"][whole])                       # a range reports the whole's points of its planes, in order


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_model_order(shape):
    """Workgroups ascending; inside one, (z, y, x, direction) ascending — the oracle's order restricted to its columns."""
    X, Y, Z = shape
    gx, gy = ec.blocks_of(shape)
    for c in cases_of(shape):
        assert np.array_equal(c["wg"], c["x"] // 64 + gx * (c["y"] // 4))
        assert (np.diff(c["wg"]) >= 0).all() and (c["wg"] < gx * gy).all()
        key = ((c["z"] * Y + c["y"]) * X + c["x"]) * 3 + c["d"]
        same = np.diff(c["wg"]) == 0
        assert (np.diff(key)[same] > 0).all()
        # and a point sits where its voxel and direction say: two coordinates are the voxel's centre
        vs = np.float32(c["vs"])
        for axis, idx in enumerate((c["x"], c["y"], c["z"])):
            fixed = c["d"] != axis
            centre = (idx.astype(np.float32) + np.float32(0.5)) * vs
            assert ec.same_bits(c["points"][fixed, axis], centre[fixed])


@pytest.mark.parametrize("name", list(ec.SMOOTH))
def test_float32_model_against_float64_twin(name):
    """Measured (largest error / bound): recorded in DESIGN.md section 4.10."""
    s = ec.smooth_case(name)
    shape, vs, v = s["shape"], s["vs"], s["value"]
    p32, n = ec.points(v, shape, vs)
    p64, n64 = ec.points(v, shape, vs, dtype=np.float64)
    assert n == n64 > 500                                                 # the predicates see the same float32 values
    perr = np.abs(p32.astype(np.float64) - p64).max()
    assert perr <= ec.point_bound(shape, vs), (perr, ec.point_bound(shape, vs))
    m32, in32, _ = ec.normals(v, shape, vs, p32, details=True)
    m64, in64, _ = ec.normals(v, shape, vs, p32, dtype=np.float64, details=True)
    assert np.array_equal(in32, in64) and in32.sum() > 300
    length = 1.0 / np.sqrt((m64[in64] ** 2).sum(axis=1))
    assert length.min() > ec.GRAD_FLOOR, length.min()
    bound = ec.normal_bound(v, shape, m64[in64])
    nerr = np.abs(m32[in32].astype(np.float64) - m64[in64]).max(axis=1)
    print(f"{name} {shape}: points {n}, max point error {perr:.3e} (bound {ec.point_bound(shape, vs):.3e}); normals {int(in32.sum())}, "
          f"max normal error {nerr.max():.3e}, max error / bound {(nerr / bound).max():.4f}, shortest |n| {length.min():.3f}")
    assert (nerr <= bound).all(), (nerr / bound).max()
    assert (m32[~in32] == 0).all() and (m64[~in64] == 0).all()


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=str)
def test_case_conditions(shape):
    X, Y, Z = shape
    c = ec.random_case(shape)
    counts = ec.crossing_counts(c)
    if counts.size >= 64:                                                 # (2, 2, 2) has one candidate voxel
        assert all((counts == k).any() for k in (0, 1, 2, 3)), [int((counts == k).sum()) for k in range(4)]
    if counts.size >= 180:                                                # (5, 5, 5) and (6, 4, 7) hold a handful of each edge value
        pairs = ec.edge_pairs(c)
        for name, (acc, rej) in pairs.items():
            e = ec.EDGE_VALUES[name]
            if e >= ec.LIMIT or e == 0:
                assert acc == 0 and rej > 0, (name, acc, rej)             # never accepted; rejected for this value alone
            else:
                assert acc > 0 and rej > 0, (name, acc, rej)
    one, three = ec.full_ballots(c)
    if X >= 65:
        assert one >= 2 and (three >= 1 or Y < 3 or Z < 3), (one, three)
        assert (counts[:, :, 63] > 0).any()                               # lane 63 reports: the mask below it has 63 bits
    gx, gy = ec.blocks_of(shape)
    if shape in ec.SCAN_SHAPES:
        assert gx * gy == ec.SCAN_SHAPES[shape]
        nonempty = np.bincount(c["wg"], minlength=gx * gy) > 0
        assert nonempty[::gx].all()                                       # every workgroup with a reporting column has points
        s = ec.sparse_case(shape)
        filled = set(np.unique(s["wg"]).tolist())
        assert filled <= {0, 255, 256, 257, gx * gy - 2, gx * gy - 1} and 0 in filled and len(filled) >= 2
        assert 0 < s["found"] < c["found"] // 20
    # normals: an interior exists exactly where every dimension exceeds 4
    interior = min(shape) > 4
    assert bool(c["general_inner"].any()) == interior
    nz = (c["general_normals"] != 0).any(axis=1)
    assert not (nz & ~c["general_inner"]).any()
    if interior:
        assert nz[c["general_inner"]].mean() > 0.9
        assert len(c["general"]) % 256 != 0 and len(c["general"]) > 4000
    else:
        assert not nz.any() and not (c["normals"] != 0).any()


def test_empty_case_finds_nothing():
    assert ec.empty_case((2, 2, 2))["found"] == 0


def test_capacities_cut_where_they_say():
    for shape in ((65, 9, 7), (33, 1028, 3)):
        c = ec.random_case(shape)
        caps = ec.capacities(c)
        assert caps[0] == 0 and caps[1] == 1 and caps[4:] == [c["found"] - 1, c["found"], c["found"] + 5]
        k = caps[2]
        assert (c["z"][k - 2], c["y"][k - 2], c["x"][k - 2]) == (c["z"][k], c["y"][k], c["x"][k]) and c["d"][k] == 2
        assert 0 < caps[3] < c["found"] and c["wg"][caps[3]] != c["wg"][caps[3] - 1]
    assert ec.random_case((33, 1028, 3))["wg"][ec.capacities(ec.random_case((33, 1028, 3)))[3]] == 256
