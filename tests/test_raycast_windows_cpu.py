"""CPU, oracle only: the inputs of tests/test_raycast_windows_gpu.py are what that test takes them for.  The window identity is a
property of the operation (the oracle's raycast of every window is the crop of its full-frame raycast, bit for bit), the windows
hold the hits recorded in raycast_cases.WINDOWS, and the three-slab setting exercises the composite: no read outside the stored
planes, no key ties, the owner composite equal to the window's raycast, two slabs owning a large share of windows C and D, and
pixels of every kind (vertex, event without vertex, no event) in window A."""
import numpy as np
import pytest

import raycast_cases as rc

IDS = list(rc.WINDOWS)


@pytest.fixture(scope="module")
def s(oracle):
    return rc.setting(oracle)


def test_setting_has_a_surface_in_view(s):
    assert s["full_hits"] > 0.5 * rc.H * rc.W
    assert s["full_hits"] == int(rc.valid_of(s["full_v"], rc.H).sum())


@pytest.mark.parametrize("wid", IDS)
def test_oracle_window_is_the_crop_of_the_full_frame(oracle, s, wid):
    win, want_hits = rc.WINDOWS[wid]
    rows = win[2]
    vm, nm, hits = rc.oracle_window(oracle, s, win)
    cv, cn = rc.crop(s["full_v"], win), rc.crop(s["full_n"], win)
    assert np.array_equal(vm.view(np.int32), cv.view(np.int32)) and np.array_equal(nm.view(np.int32), cn.view(np.int32))
    assert rc.assert_same_maps(vm, nm, cv, cn, rows, wid) == hits == want_hits


@pytest.mark.parametrize("wid", IDS)
def test_oracle_slab_composite_is_the_window(oracle, s, wid):
    win, want_hits = rc.WINDOWS[wid]
    rows, cols = win[2:]
    parts, bad = rc.oracle_slabs(oracle, s, win)
    assert bad == 0                                                       # the 6-plane halo suffices
    keys = np.stack([p[2] for p in parts])
    for i in range(len(parts)):
        for j in range(i + 1, len(parts)):
            assert not ((keys[i] == keys[j]) & (keys[i] != rc.INT_MAX)).any()    # a step is one slab's
    vm, nm, mk, mine = rc.compose_numpy(parts, rows, cols)
    wv, wn, hits = rc.oracle_window(oracle, s, win)
    assert rc.assert_same_maps(vm, nm, wv, wn, rows, wid) == hits == want_hits
    assert int(mine.sum()) == hits and (mine.sum(axis=0) <= 1).all()
    if wid in rc.TWO_OWNERS:
        assert int((mine.sum(axis=1) > 1000).sum()) >= 2, mine.sum(axis=1)
    if wid == "A":
        assert int((((mk & 1) == 1) & (mk != rc.INT_MAX)).sum()) == 1175 and int((mk == rc.INT_MAX).sum()) == 380
