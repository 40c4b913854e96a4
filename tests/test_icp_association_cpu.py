"""The numpy model of the ICP reduction's association (tests/icp_association.py) against a plain Python loop over the same
records, one double at a time: the model is what tests/test_icp_association_gpu.py holds the device against bit for bit."""
import numpy as np
import pytest

from icp_association import RECORD_DOUBLES, SUMS, device_sum, index_order_sum, row_groups


def _records(count, seed):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((count, RECORD_DOUBLES)) * 1e3
    r[:, 54] = rng.integers(0, 1216, count)                       # inlier counts
    r[:, 55] = 7.0                                                # the pad / sequence word: never part of a sum
    r[count // 3] = -0.0                                          # a workgroup whose pixels were all rejected, signed zeros
    r[count // 2, :54] = np.ldexp(rng.standard_normal(54), rng.integers(-30, 31, 54))   # a 2^60 spread of magnitudes in one record
    return r


def _loop_device(r, G):
    out = []
    for k in range(SUMS):
        groups = []
        for g in range(G):
            s = 0.0
            b = g
            while b < len(r):
                s = s + float(r[b][k])
                b += G
            groups.append(s)
        t = groups[0]
        for g in range(1, G):
            t = t + groups[g]
        out.append(t)
    return np.array(out, np.float64)


def _loop_index(r):
    out = []
    for k in range(SUMS):
        s = 0.0
        for b in range(len(r)):
            s = s + float(r[b][k])
        out.append(s)
    return np.array(out, np.float64)


@pytest.mark.parametrize("count,G", [(45, 18), (150, 18), (256, 36), (375, 18), (512, 9)])
def test_model_adds_like_a_plain_loop(count, G):
    r = _records(count, 1000 + count)
    got, want = device_sum(r, G), _loop_device(r.tolist(), G)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    got, want = index_order_sum(r), _loop_index(r.tolist())
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # the order matters at these magnitudes: the two associations are not the same sum
    assert not np.array_equal(device_sum(r, G), index_order_sum(r))
    assert not np.array_equal(device_sum(r, G), device_sum(r, 2 * G if G < 36 else 18))


def test_zero_records_and_missing_groups():
    """All-(-0.0) records add up to +0.0 (every chain starts from +0.0), and a launch with fewer records than row groups adds the empty
    groups' +0.0 all the same."""
    r = np.full((5, RECORD_DOUBLES), -0.0)
    for G in (9, 18, 36):
        s = device_sum(r, G)
        assert not s.any() and not np.signbit(s).any()
    assert not np.signbit(index_order_sum(r)).any()
    r = _records(5, 7)
    assert np.array_equal(device_sum(r, 18).view(np.uint64), _loop_device(r.tolist(), 18).view(np.uint64))


def test_row_groups_follow_the_launch_shapes():
    assert [row_groups(640, 480), row_groups(320, 240), row_groups(160, 120)] == [36, 18, 18]
    assert row_groups(640, 300) == 18 and row_groups(1024, 448) == 9 and row_groups(1280, 960) == 9
