"""GPU: the HIP map-preparation kernels (x-slam_amd/csrc/xs_map.hip), through the C ABI, against the independently written float64
model of tests/independent_f64.py: the cases of tests/map_cases.py — small ragged images, three pitches per side, guard rows, the
bilateral filter's tie-zone rule and dead pixels, the pyramid's gate and rounding, vertex / normal maps and resizes with their
derivatives, and the fused launches.  Measured figures are written to maps_independent_f64.json in the directory XS_FIGURES_DIR names, when it is set (a recorded run:
profiles/maps_independent_f64.json)."""
import importlib
import json
import os

import pytest

import independent_cases as ic
import map_cases as mc

pytestmark = pytest.mark.gpu
SHAPES = [pytest.param(r, c, id=f"{r}x{c}") for r, c in mc.SHAPES]
LOG = {}


@pytest.fixture(scope="module")
def be():
    import torch
    assert torch.cuda.is_available()
    capi = importlib.import_module("x-slam_amd.capi")
    yield ic.GpuBackend(torch, capi, None)
    out = os.environ.get("XS_FIGURES_DIR", "")
    if os.path.isdir(out) and LOG:
        json.dump(LOG, open(os.path.join(out, "maps_independent_f64.json"), "w"), indent=1)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_bilateral_and_its_pyramid(be, rows, cols):
    mc.check_bilateral_inputs(rows, cols)
    r, level0 = mc.check_bilateral(be, rows, cols)
    r["pyramid_levels"] = mc.check_pyramid_of_bilateral(be, level0)
    LOG[f"bilateral_{rows}x{cols}"] = r


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_pyr_down_gate_and_rounding(be, rows, cols):
    mc.check_pyr_down(be, mc.pyr_crafted(rows, cols, 3 * rows + cols))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_vertex_map(be, rows, cols):
    r = mc.check_vertex(be, rows, cols)
    LOG[f"vertex_{rows}x{cols}"] = r
    assert r["holes"] > 0


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_normal_map(be, rows, cols):
    r = mc.check_normal(be, rows, cols)
    LOG[f"normal_{rows}x{cols}"] = r
    if (rows, cols) in ((37, 70), (66, 200)):
        assert r["n_valid"] > 100 and r["kappa_max"] > 100, r


@pytest.mark.parametrize("rows,cols", SHAPES + [pytest.param(6, 6, id="6x6")])
def test_resize_maps_two_levels(be, rows, cols):
    r = mc.check_resize(be, rows, cols)
    LOG[f"resize_{rows}x{cols}"] = r
    if rows >= 6 and cols >= 6:
        assert r["nan_positions"] == 4 and "vmap_level2" in r, r


@pytest.mark.parametrize("real", [False, True])
def test_fused_vertex_normal_maps(be, real):
    LOG[f"vnmaps{'_real' if real else ''}"] = mc.check_vnmaps(be, real)


def test_fused_resize_pyramid(be):
    LOG["resize_pyramid"] = mc.check_resize_pyramid(be)
