"""CPU: the model of tests/diff_cases.py (map differencing) held to the properties the contract implies, and the case
table held to being worth running: the packer round-trips, a map differs from itself nowhere, swapping the maps swaps the classes, lo = hi
leaves no compared voxel with its two values on opposite sides unclassified, and no class of the table is empty."""
import numpy as np
import pytest

import diff_cases as dc
import frontier_cases as fc
import merge_cases as mc


@pytest.mark.parametrize("dshape,sshape", dc.SHAPES)
def test_packer_round_trips(dshape, sshape):
    for X, Y, Z in (dshape, sshape):
        rng = np.random.default_rng(X + 1000 * Y + 1000000 * Z)
        for mask in (rng.random((Z, Y, X)) < 0.4, np.ones((Z, Y, X), bool), np.zeros((Z, Y, X), bool)):
            words = dc.pack(mask)
            assert words.dtype == np.uint64 and words.shape == (dc.mask_words((X, Y, Z)),)
            back, clear = dc.unpack(words, mask.shape)
            assert clear and np.array_equal(back, mask)
            assert int(sum(bin(int(w)).count("1") for w in words)) == int(mask.sum())        # nothing in the overhang
        # one voxel: its word and its bit
        x, y, z = X - 1, Y - 1, Z - 1
        one = np.zeros((Z, Y, X), bool)
        one[z, y, x] = True
        words = dc.pack(one)
        BX, BY = (X + 3) // 4, (Y + 3) // 4
        b = ((z // 4) * BY + y // 4) * BX + x // 4
        assert int(words[b]) == 1 << ((x & 3) + 4 * (y & 3) + 16 * (z & 3)) and np.count_nonzero(words) == 1
        # a set overhang bit is reported
        if X % 4:
            words = dc.pack(np.zeros((Z, Y, X), bool))
            words[BX - 1] = np.uint64(1) << np.uint64(3)                                     # lx = 3 of the last brick along x: x = 4 BX - 1 >= X
            assert not dc.unpack(words, (Z, Y, X))[1]


@pytest.mark.parametrize("dshape,sshape", dc.SHAPES)
def test_a_map_differs_from_itself_nowhere(dshape, sshape):
    this, _ = dc.volumes(dshape, sshape)
    for mw in dc.MIN_WEIGHTS:
        a, b, counts = dc.diff(this, this, mc.xform(), mw)
        assert not a.any() and not b.any()
        assert counts == (int((this[1] >= mw).sum()), 0, 0)


@pytest.mark.parametrize("shape", [(7, 7, 7), (4, 4, 4), (9, 9, 9)])
def test_swapping_the_maps_swaps_the_masks(shape):
    """Under the identity and the 24 exact signed permutations between two cubes: B against A under the inverse map is A against B with the
    classes exchanged, voxel for voxel under the map."""
    rng = np.random.default_rng(sum(shape))
    A, B = mc.volume(rng, shape), mc.volume(rng, shape)
    n = shape[0]
    X = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), axis=-1).reshape(-1, 3)      # destination voxels (x, y, z)
    seen = 0
    for P in [np.eye(3)] + mc.signed_permutations():
        m = mc.permutation_map(P, shape)
        off = m[9:].astype(np.float64)
        inv = mc.xform(P.T, -P.T @ off)
        G = (X @ P.T + off).astype(np.int64)                                                                      # their source voxels
        assert ((G >= 0) & (G < n)).all()
        for mw in dc.MIN_WEIGHTS:
            ta, oa, ca = dc.diff(A, B, m, mw)
            tb, ob, cb = dc.diff(B, A, inv, mw)
            assert ca == (cb[0], cb[2], cb[1])
            assert np.array_equal(ta[X[:, 2], X[:, 1], X[:, 0]], ob[G[:, 2], G[:, 1], G[:, 0]])
            assert np.array_equal(oa[X[:, 2], X[:, 1], X[:, 0]], tb[G[:, 2], G[:, 1], G[:, 0]])
            seen += ca[1] + ca[2]
    assert seen > 0


@pytest.mark.parametrize("dshape,sshape", dc.SHAPES[1:5])
def test_lo_equal_to_hi_leaves_no_opposite_pair_unclassified(dshape, sshape):
    this, other = dc.volumes(dshape, sshape)
    for name in ("identity", "half_x", "rotation_10", "shift_mixed"):
        for t in (0.0, 0.25, -0.5):
            a, b, counts, d = dc.diff(this, other, dc.maps(dshape, sshape)[name], 1, lo=t, hi=t, details=True)
            t32 = np.float32(t)
            opposite = d["compared"] & ((d["v"] < t32) != (d["s"] < t32))
            assert np.array_equal(a | b, opposite) and not (a & b).any()
            assert np.array_equal(a, d["compared"] & (d["v"] < t32) & (d["s"] >= t32))


def test_minus_zero_is_not_below_zero():
    v = np.array([[[-0.0, -0.0, 0.0, -1e-30]]], np.float32)
    s = np.array([[[1.0, 0.5, 1.0, 1.0]]], np.float32)
    w = np.ones((1, 1, 4), np.int32)
    a, b, counts = dc.diff((v, w), (s, w), mc.xform())
    assert a.reshape(-1).tolist() == [False, False, False, True] and not b.any() and counts == (4, 1, 0)
    a, b, counts = dc.diff((s, w), (v, w), mc.xform())
    assert b.reshape(-1).tolist() == [False, False, False, True] and not a.any()


def test_the_case_table_is_not_vacuous():
    """Every shape pair from (64, 4, 2) upward has compared, only_this and only_other voxels under the exact maps, at both min_weights; the map
    that misses the source compares nothing, anywhere."""
    for dshape, sshape in dc.SHAPES:
        for mw in dc.MIN_WEIGHTS:
            assert dc.expected(dshape, sshape, "miss", mw)[2] == (0, 0, 0)
            assert not dc.expected(dshape, sshape, "miss", mw)[0].any() and not dc.expected(dshape, sshape, "miss", mw)[1].any()
    for dshape, sshape in dc.SHAPES[2:]:
        for name in dc.NONVACUOUS_MAPS:
            for mw in dc.MIN_WEIGHTS:
                counts = dc.expected(dshape, sshape, name, mw)[2]
                assert min(counts) > 0, (dshape, sshape, name, mw, counts)
    assert dc.expected((65, 9, 7), (63, 3, 5), "identity", 1)[2] == (526, 49, 64)
    assert dc.expected((64, 4, 2), (64, 4, 2), "identity", 3)[2] == (179, 16, 16)


def test_clusters_of_a_mask():
    """The cluster model on a mask that is no frontier: two blobs that touch across a cell boundary are one cluster with cell 0 and two with cell 8."""
    mask = np.zeros((4, 12, 20), bool)
    mask[1, 2, 6:10] = True                      # x 6 .. 9 crosses x = 8
    mask[3, 11, 19] = True
    r0, r8 = dc.clusters(mask, 0), dc.clusters(mask, 8)
    assert r0[:, 1].tolist() == [4, 1] and r8[:, 1].tolist() == [2, 2, 1]
    assert r0[0, 0] == (1 * 12 + 2) * 20 + 6 and r0[0, 2:5].tolist() == [6 + 7 + 8 + 9, 8, 4]
    assert (fc.unpack_box(r0[0][5]), fc.unpack_box(r0[0][6])) == ((6, 2, 1), (9, 2, 1))
    assert len(dc.select(r0, 2)) == 1 and len(dc.select(r8, 2)) == 2 and len(dc.select(r8, 3)) == 0

