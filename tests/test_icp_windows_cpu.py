"""CPU: the oracle's ICP reduction (oracle/oc_kernels.hpp: icp_combined) against the independently written float64 model of
tests/independent_f64.py on the geometries of tests/icp_cases.py — the smallest images that reach each instance of the HIP kernel and
each of its edges, in pitched buffers with guard rows, whole and by row ranges.  The oracle is complex<float> in the reference's
operation order, so this is also the check that the derived tolerances are right.  The same cases run against the HIP kernels in
tests/test_icp_windows_gpu.py."""
import importlib

import pytest

import icp_cases as icp
import independent_cases as ic
from icp_association import row_groups

SHAPES = [pytest.param(r, c, id=f"{r}x{c}") for r, c in icp.SHAPES]


@pytest.fixture(scope="module")
def be(oracle):
    return ic.OracleBackend(oracle)


@pytest.mark.parametrize("rows,cols,tiles,records,G", [pytest.param(*g[:5], id=f"{g[0]}x{g[1]}") for g in icp.GEOMETRIES])
def test_geometry_reaches_its_instance(rows, cols, tiles, records, G):
    """The launch shapes the table states: tiles, records (xs_icp_records_count is host code) and the gather's row groups."""
    capi = importlib.import_module("x-slam_amd.capi")
    assert -(-cols // 64) * rows == tiles
    assert capi.icp_records_count(cols, 0, rows) == records and row_groups(cols, rows) == G
    for y0, y1 in icp.RANGES.get((rows, cols), []):
        assert row_groups(cols, rows, y0, y1) == (36 if 4096 < -(-cols // 64) * (y1 - y0) <= 5120 else 18)
    if (rows, cols) == (1500, 130):
        assert [capi.icp_records_count(cols, *r) for r in icp.RANGES[(rows, cols)]] == [256, 19, 19]
        assert [row_groups(cols, rows, *r) for r in icp.RANGES[(rows, cols)]] == [36, 18, 18]
    if (rows, cols) == icp.EMPTY_SHAPE:
        assert [capi.icp_records_count(cols, *r) for r in icp.EMPTY_RANGES] == [1, 1, 1]


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_inputs_hold_every_branch_and_no_fragile_pixel(rows, cols):
    """Each rejection branch has members, the pixels that idle lanes read are inliers, no decision is left within the float32 error of
    its boundary, and the pixels punched out for that are at most 5 % of the current pixels with a valid normal."""
    print(icp.check_inputs(rows, cols))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_sums_and_inliers(be, rows, cols):
    icp.check_inputs(rows, cols)
    r, _ = icp.check_case(be, rows, cols)
    print(rows, cols, r)


@pytest.mark.parametrize("rows,cols", [pytest.param(r, c, id=f"{r}x{c}") for r, c in icp.RANGES])
def test_row_ranges(be, rows, cols):
    print(rows, cols, icp.check_ranges(be, rows, cols))


def test_empty_ranges(be):
    icp.check_empty(be)


@pytest.mark.parametrize("rows,cols", [pytest.param(r, c, id=f"{r}x{c}") for r, c in icp.ALL_PITCHES + icp.POSTED_SHAPES[1:]])
def test_real_planes_stand_for_zero_imaginary_parts(be, rows, cols):
    """The inputs of the _real entry points: float planes and complex maps with zero imaginary parts give the same 55 doubles."""
    c = icp.case(rows, cols)
    for kind in (0, 1, 2) if (rows, cols) in icp.ALL_PITCHES else (1,):
        a, b = icp.run(be, c, kind, real=True), icp.run(be, c, kind, real=True)
        maps, _ = icp.buffers(c, kind, real=True)
        plain = be.icp_p(c["Rcurr"], c["tcurr"], maps[0], maps[1], c["Rprev_inv"], c["tprev"], c["intr"], maps[2], maps[3], rows, cols, icp.DIST, icp.ANGLE)
        assert a.tobytes() == b.tobytes() == plain.tobytes() and a[54] == c["whole"]["inliers"]
