"""GPU: the HIP ICP reduction (x-slam_amd/csrc/xs_icp.hip), through the C ABI, against the independently written float64 model of
tests/independent_f64.py on the geometries of tests/icp_cases.py: the smallest images that reach each instance of k_icp and each of
its edges (one row, one column, tail tiles of three and six lanes, the first and last launch of every instance, both ends of the
balanced partition), in pitched buffers whose guard rows and padding hold data and must come back untouched; whole images and row
ranges, empty ones included.  Then, per geometry, the entry points against each other bit for bit (the float-plane form, the records
and their host fold, the last workgroup's gather against tests/icp_association.py, a repeated launch, the posted pose).
Measured figures are written to icp_windows_f64.json in the directory XS_FIGURES_DIR names, when it is set, as tests/test_maps_gpu.py
does (a recorded run: profiles/icp_windows_f64.json)."""
import importlib
import json
import os

import numpy as np
import pytest

import icp_cases as icp
import independent_cases as ic
from icp_association import device_sum, index_order_sum

pytestmark = pytest.mark.gpu
SHAPES = [pytest.param(r, c, id=f"{r}x{c}") for r, c in icp.SHAPES]
LOG = {}


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    capi = importlib.import_module("x-slam_amd.capi")
    yield ic.GpuBackend(torch, capi, None)
    out = os.environ.get("XS_FIGURES_DIR", "")
    if os.path.isdir(out) and LOG:
        json.dump(LOG, open(os.path.join(out, "icp_windows_f64.json"), "w"), indent=1)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_sums_and_inliers(be, rows, cols):
    icp.check_inputs(rows, cols)
    r, _ = icp.check_case(be, rows, cols)
    LOG[f"whole_{rows}x{cols}"] = r


@pytest.mark.parametrize("rows,cols", [pytest.param(r, c, id=f"{r}x{c}") for r, c in icp.RANGES])
def test_row_ranges(be, rows, cols):
    LOG[f"ranges_{rows}x{cols}"] = icp.check_ranges(be, rows, cols)


@pytest.mark.parametrize("form", ["device", "pairs", "records"])
def test_empty_ranges(be, form):
    """55 zeros from (0, 0), (k, k) and (rows, rows), and every publishing form completes."""
    icp.check_empty(be, form=form)


@pytest.mark.parametrize("rows,cols,records,G", [pytest.param(g[0], g[1], g[3], g[4], id=f"{g[0]}x{g[1]}") for g in icp.GEOMETRIES])
def test_entry_points_and_association(be, rows, cols, records, G):
    """xs_icp_accumulate twice on one workspace; xs_icp_accumulate_records + xs_icp_sum_records on the same inputs — the host fold is
    the index-order sum of the records, and the device's result is the model of the last workgroup's gather applied to them (1, 2, 5,
    10, 60 records: fewer than one per row group or a tail only; 256 .. 768: the full-batch loop and its tail); xs_icp_accumulate_real
    on float planes against xs_icp_accumulate on the same maps with zero imaginary parts.  All bit for bit."""
    c = icp.case(rows, cols)
    for kind in (0, 1, 2) if (rows, cols) in icp.ALL_PITCHES else (1,):
        plain = icp.run(be, c, kind, launches=2)
        host = icp.run(be, c, kind, form="records")
        rec = be.records
        assert rec.shape == (records, 56) and np.array_equal(rec[:, 55].view(np.uint64), np.full(records, 11, np.uint64))
        assert rec[:, 54].sum() == c["whole"]["inliers"]
        assert same_bits(host, index_order_sum(rec))
        want = device_sum(rec, G)
        assert same_bits(plain, want), np.flatnonzero(plain.view(np.uint64) != want.view(np.uint64))
        real, zero = icp.run(be, c, kind, real=True), icp.run(be, c, kind, zero=True)
        assert same_bits(real, zero) and real[54] == c["whole"]["inliers"]
        assert real.any() and not same_bits(real, plain)                  # (the imaginary parts of the current maps are in the sums)


@pytest.mark.parametrize("rows,cols", [pytest.param(r, c, id=f"{r}x{c}") for r, c in icp.POSTED_SHAPES])
def test_posted_pose(be, rows, cols):
    """xs_icp_accumulate_posted and _posted_real: the pose is posted before anything synchronises; the same bits as the launch that
    takes its pose as an argument."""
    c = icp.case(rows, cols)
    assert same_bits(icp.run(be, c, 1, posted=True), icp.run(be, c, 1))
    assert same_bits(icp.run(be, c, 1, real=True, posted=True), icp.run(be, c, 1, real=True))
