"""The ICP reduction's additions, bit for bit: the 55 doubles of xs_icp_accumulate (the last workgroup adds the per-workgroup records
on the device) against the float64 model of that association (tests/icp_association.py) applied to the same launch's records, which
xs_icp_accumulate_records delivers to the host; and xs_icp_sum_records against an index-order sum of them.  One shape per kernel
instance and per path through the two chains: the three levels of a 640 x 480 frame (256 sixteen-wave records: 36 row groups;
150 and 45 one-pass eight-wave records: 18), 640 x 300 (375 two-pass eight-wave records: the gather's full-batch loop and its tail)
and 1024 x 448 (7 168 tiles, 512 four-wave records: 9 row groups)."""
import ctypes as C
import importlib

import numpy as np
import pytest

from helpers import intr_of, synth
from icp_association import RECORD_DOUBLES, device_sum, index_order_sum, row_groups
from test_kernels_gpu import _coherent_host_bytes, icp_inputs, to_dev

pytestmark = pytest.mark.gpu
H, W = synth.HEIGHT, synth.WIDTH


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi")


@pytest.fixture(scope="module")
def inputs(oracle):
    """The maps of every case, made once: {name: (rows, cols, intrinsics, cv, cn, pv, pn)} and the pose."""
    prm, T0, pv, pn, cv, cn = icp_inputs(oracle)
    cases = {}
    planes = lambda m, h, w: m.reshape(3, h, w, 2)
    k = np.asarray(intr_of(prm), np.float32).copy()
    cases["level0_640x480"] = (H, W, k, cv, cn, pv, pn)
    rows, cols = 300, W
    f = lambda m: np.ascontiguousarray(planes(m, H, W)[:, :rows, :cols]).reshape(3 * rows, cols, 2)
    cases["crop_640x300"] = (rows, cols, k, f(cv), f(cn), f(pv), f(pn))
    rows, cols = 448, 1024
    f = lambda m: np.ascontiguousarray(np.repeat(np.repeat(planes(m, H, W), 2, axis=1), 2, axis=2)[:, :rows, :cols]).reshape(3 * rows, cols, 2)
    cases["double_1024x448"] = (rows, cols, (k * 2).astype(np.float32), f(cv), f(cn), f(pv), f(pn))
    d = oracle.bilateral(synth.s1_frame(1))
    lpv, lpn = pv, pn
    for level in (1, 2):
        lpv, lpn = oracle.resize_map(lpv, False), oracle.resize_map(lpn, True)
        d = oracle.pyr_down(d)
        lk = intr_of(prm, level)
        lcv = oracle.create_vmap(lk, d)
        lcn = oracle.create_nmap(lcv)
        cases[f"level{level}_{W >> level}x{H >> level}"] = (lcv.shape[0] // 3, lcv.shape[1], lk, lcv, lcn, lpv, lpn)
    return T0, cases


@pytest.mark.parametrize("name,count,G", [("level0_640x480", 256, 36), ("level1_320x240", 150, 18), ("level2_160x120", 45, 18),
                                          ("crop_640x300", 375, 18), ("double_1024x448", 512, 9)])
def test_device_sums_follow_the_model_bit_for_bit(dev, oracle, inputs, name, count, G):
    torch, capi = dev
    T0, cases = inputs
    rows, cols, k, cv, cn, pv, pn = cases[name]
    assert capi.icp_records_count(cols, 0, rows) == count and row_groups(cols, rows) == G
    Rprev_inv = oracle.m3_inverse(T0["Rc2w"])
    angle = float(np.sin(np.float32(15.0) / np.float32(180.0) * np.pi))
    dv = [to_dev(torch, x) for x in (cv, cn, pv, pn)]
    rec, free = _coherent_host_bytes(capi.icp_records_bytes())
    try:
        capi.icp_accumulate_records(T0["Rc2w"], T0["tc2w"], dv[0], dv[1], Rprev_inv, T0["tc2w"], k, dv[2], dv[3], cols * 8, rows, cols, 0.10, angle, rec, 5)
        rc, host_sums = capi.icp_sum_records(rec, count, 5)
        assert rc == 0
        torch.cuda.synchronize()
        records = np.ctypeslib.as_array((C.c_double * (count * RECORD_DOUBLES)).from_address(rec)).reshape(count, RECORD_DOUBLES).copy()
    finally:
        free()
    assert records[:, 54].sum() > 0.3 * rows * cols and np.count_nonzero(records[:, :54]) > 40 * count      # real work in every sum
    assert np.array_equal(records[:, 55].view(np.uint64), np.full(count, 5, np.uint64))                     # the sequence word, not a sum
    # the host fold: index order
    assert np.array_equal(host_sums.view(np.uint64), index_order_sum(records).view(np.uint64))
    # the device's last workgroup: row groups, then group order — from the same records (the record is the same code on both paths)
    ws = torch.zeros(capi.icp_workspace_bytes(), dtype=torch.uint8, device="cuda")
    sums = torch.zeros(55, dtype=torch.float64, device="cuda")
    capi.icp_accumulate(T0["Rc2w"], T0["tc2w"], dv[0], dv[1], Rprev_inv, T0["tc2w"], k, dv[2], dv[3], cols * 8, rows, cols, 0.10, angle, ws, sums)
    torch.cuda.synchronize()
    got = sums.cpu().numpy()
    want = device_sum(records, G)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    # and the association is visible in these sums: the index-order fold of the same records is another double somewhere
    assert not np.array_equal(got, host_sums)
