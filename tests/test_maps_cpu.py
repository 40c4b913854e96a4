"""CPU: the oracle's map-preparation kernels (bilateral filter, depth pyramid, vertex / normal maps, resizes; oracle/oc_kernels.hpp)
against the independently written float64 model of tests/independent_f64.py, on small ragged images in pitched buffers with guard
rows (tests/map_cases.py).  The same cases run against the HIP kernels in tests/test_maps_gpu.py."""
import pytest

import independent_cases as ic
import map_cases as mc

SHAPES = [pytest.param(r, c, id=f"{r}x{c}") for r, c in mc.SHAPES]


@pytest.fixture(scope="module")
def be(oracle):
    return ic.OracleBackend(oracle)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_bilateral_inputs_are_unambiguous(rows, cols):
    """The generator's guarantees (no weight near float32 underflow; dead, in-range and flushed pixels present), the float32
    emulation's deviation against TAU, and the tie-zone share against its cap."""
    mc.check_bilateral_inputs(rows, cols)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_bilateral_and_its_pyramid(be, rows, cols):
    _, level0 = mc.check_bilateral(be, rows, cols)
    mc.check_pyramid_of_bilateral(be, level0)


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_pyr_down_gate_and_rounding(be, rows, cols):
    mc.check_pyr_down(be, mc.pyr_crafted(rows, cols, 3 * rows + cols))


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_vertex_map(be, rows, cols):
    r = mc.check_vertex(be, rows, cols)
    assert r["holes"] > 0


@pytest.mark.parametrize("rows,cols", SHAPES)
def test_normal_map(be, rows, cols):
    r = mc.check_normal(be, rows, cols)
    assert 4 * r["model_f32_spread"] <= mc.C_MAP, r
    if (rows, cols) in ((37, 70), (66, 200)):
        assert r["n_valid"] > 100 and r["kappa_max"] > 100, r             # the 0.5 m corners are there


@pytest.mark.parametrize("rows,cols", SHAPES + [pytest.param(6, 6, id="6x6")])
def test_resize_maps_two_levels(be, rows, cols):
    r = mc.check_resize(be, rows, cols)
    assert all(4 * f["model_f32_spread"] <= mc.C_MAP for k, f in r.items() if k != "nan_positions"), r
    if rows >= 6 and cols >= 6:
        assert r["nan_positions"] == 4 and "vmap_level2" in r, r


@pytest.mark.parametrize("real", [False, True])
def test_fused_vertex_normal_maps(be, real):
    mc.check_vnmaps(be, real)


def test_fused_resize_pyramid(be):
    mc.check_resize_pyramid(be)
