"""GPU: the raycast kernels and the slab composite (x-slam_amd/csrc/xs_raycast.hip) on ragged image windows.  Every other raycast
test launches 640 x 480, where every tile is full, no workgroup is idle, the pack's last block is full and every buffer is dense.
Here each window of raycast_cases.WINDOWS is cast with the intrinsics shifted by its (integer) origin and must equal the crop of ONE
full-frame raycast bit for bit (raycast_cases: why that is exact), in every launch form: the single kernel, march + crossing, the
fused sign-map launch without and with the pyramid, and three slab marches composed both ways.  Every output lies in a pitched
buffer with guard rows (flat arrays: guard elements) filled with a pattern that has to survive.  The composite kernels are also
held against plain numpy statements on crafted keys, at sizes that take their grid-stride loops and ragged last blocks.
tests/test_raycast_windows_cpu.py shows on the oracle alone that these inputs exercise what is claimed."""
import importlib

import numpy as np
import pytest

import raycast_cases as rc
from raycast_cases import DevFlat, DevMap, H, N, W, map_pitch

pytestmark = pytest.mark.gpu
IDS = list(rc.WINDOWS)
FILL = 5.0                                    # the full-frame baselines' unwritten entries


@pytest.fixture(scope="module")
def g(oracle):
    """The volume on the device, its sign map, and the full-frame baselines every window is held against (taken once)."""
    import torch
    assert torch.cuda.is_available()
    capi = importlib.import_module("x-slam_amd.capi")
    s = rc.setting(oracle)
    value = torch.from_numpy(s["value"].copy().reshape(N * N, N)).cuda()
    grad = torch.from_numpy(s["grad"].copy().reshape(N * N, N)).cuda()
    shift = capi.raycast_signmap_shift(s["intr"], s["vs"], s["trunc"])
    assert shift != 0
    sm = torch.zeros(capi.signmap_bytes(s["res"], shift), dtype=torch.uint8, device="cuda")
    capi.signmap_rebuild(sm, s["res"], shift, s["trunc"], value, N * 4)
    new = lambda r=H, c=W: torch.full((3 * r, c, 2), FILL, dtype=torch.float32, device="cuda")
    common = (s["intr"], *s["pose"], s["trunc"], s["res"], s["vs"], value, grad, N * 4)
    vm, nm, hits = new(), new(), torch.zeros(1, dtype=torch.int64, device="cuda")
    capi.raycast(*common, vm, nm, W * 8, H, W, hits=hits)
    vm2, nm2, hits2 = new(), new(), torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(H * W, dtype=torch.float32, device="cuda")
    steps = torch.zeros(H * W, dtype=torch.int32, device="cuda")
    capi.raycast(*common, vm2, nm2, W * 8, H, W, hits=hits2, workspace=ws, steps=steps)
    pyr = [new(H // 2, W // 2), new(H // 2, W // 2), new(H // 4, W // 4), new(H // 4, W // 4)]
    capi.resize_pyramid(vm, nm, W * 8, H, W, pyr[0], pyr[1], (W // 2) * 8, pyr[2], pyr[3], (W // 4) * 8)
    torch.cuda.synchronize()
    full = dict(v=vm.cpu().numpy(), n=nm.cpu().numpy(), hits=int(hits.item()), ws=ws.cpu().numpy(), steps=steps.cpu().numpy(),
                pyr=[p.cpu().numpy() for p in pyr])
    assert full["hits"] == int(rc.valid_of(full["v"], H).sum()) and abs(full["hits"] - s["full_hits"]) <= 3     # (test_raycast's allowance)
    assert int(hits2.item()) == full["hits"]
    assert rc.assert_same_maps(vm2.cpu().numpy(), nm2.cpu().numpy(), full["v"], full["n"], H, "full frame, march + crossing") == full["hits"]
    assert (full["ws"] >= 0).sum() >= full["hits"] and full["steps"].max() > 8
    for a in full["pyr"] + [full["v"], full["n"], full["ws"], full["steps"]]:
        a.setflags(write=False)
    return dict(torch=torch, capi=capi, s=s, value=value, grad=grad, sm=sm, shift=shift, full=full)


def under_sentinel_untouched(m, rows):
    """y / z planes of a pixel whose x plane holds the sentinel were never written: they still hold the buffer's pattern"""
    img = m.image()
    bad = ~rc.valid_of(img, rows)
    return bool((img.reshape(3, rows, -1, 2)[1:, bad].view(np.uint8) == rc.PATTERN).all())


def cast(g, wid, workspace=False, signmap=False, pyramid=False):
    """One window in one launch form, into guarded buffers; guards, maps, hit count (and crossing times / march lengths where the form
    gives them) checked against the crop of the full frame.  Returns the buffers."""
    torch, capi, s, full = g["torch"], g["capi"], g["s"], g["full"]
    win, oracle_hits = rc.WINDOWS[wid]
    y0, x0, rows, cols = win
    what = (wid, "workspace" if workspace else "single kernel", "sign map" if signmap else "", "pyramid" if pyramid else "")
    vm, nm = DevMap(torch, 3 * rows, cols, map_pitch(cols)), DevMap(torch, 3 * rows, cols, map_pitch(cols))
    hits = torch.zeros(1, dtype=torch.int64, device="cuda")
    kw, out = {}, dict(vm=vm, nm=nm)
    if workspace:
        out["ws"], out["steps"] = DevFlat(torch, rows * cols, torch.float32), DevFlat(torch, rows * cols, torch.int32)
        kw.update(workspace=out["ws"].t, steps=out["steps"].t)
    if signmap:
        kw.update(signmap=g["sm"], signmap_shift=g["shift"], signmap_tranc_dist=s["trunc"])
    if pyramid:
        r1, c1, r2, c2 = rows // 2, cols // 2, rows // 4, cols // 4
        out["pyr"] = [DevMap(torch, 3 * r1, c1, c1 * 8 + 24), DevMap(torch, 3 * r1, c1, c1 * 8 + 24),
                      DevMap(torch, 3 * r2, c2, c2 * 8 + 8), DevMap(torch, 3 * r2, c2, c2 * 8 + 8)]
        p = out["pyr"]
        kw.update(pyramid=(p[0].addr, p[1].addr, p[0].pitch, p[2].addr, p[3].addr, p[2].pitch))
    o = capi.raycast(rc.window_intr(s["intr"], y0, x0), *s["pose"], s["trunc"], s["res"], s["vs"], g["value"], g["grad"], N * 4,
                     vm.addr, nm.addr, vm.pitch, rows, cols, hits=hits, **kw)
    torch.cuda.synchronize()
    out["opts"] = o
    for name, b in out.items():
        for x in (b if isinstance(b, list) else [b]):
            if isinstance(x, (DevMap, DevFlat)):
                assert x.outside_untouched(), (what, name, "a store outside the image")
    cv, cn = rc.crop(full["v"], win), rc.crop(full["n"], win)
    n_valid = rc.assert_same_maps(vm.image(), nm.image(), cv, cn, rows, what)
    assert under_sentinel_untouched(vm, rows) and under_sentinel_untouched(nm, rows), what
    assert int(hits.item()) == n_valid, what                              # the crop's own count: exact
    assert abs(n_valid - oracle_hits) <= 3, what                          # what test_raycast allows between GPU and oracle
    if workspace:
        assert np.array_equal(out["ws"].host().view(np.int32).reshape(rows, cols), rc.crop(full["ws"], win).view(np.int32)), (what, "crossing times")
        assert np.array_equal(out["steps"].host().reshape(rows, cols), rc.crop(full["steps"], win)), (what, "march lengths")
    return out


@pytest.mark.parametrize("wid", IDS)
def test_single_kernel(g, wid):
    cast(g, wid)


@pytest.mark.parametrize("wid", IDS)
def test_march_and_crossing_kernels(g, wid):
    cast(g, wid, workspace=True)


@pytest.mark.parametrize("wid", IDS)
def test_fused_sign_map_launch(g, wid):
    cast(g, wid, workspace=True, signmap=True)


@pytest.mark.parametrize("wid", IDS)
def test_fused_launch_with_the_pyramid(g, wid):
    """Levels 1 and 2 from the raycast's own workgroups against xs_resize_pyramid on this window's level 0 (in buffers of other
    pitches); for origins that are multiples of 4 also against the crops of the full frame's pyramid.  A level without rows or
    columns (windows F, G, H) leaves its buffer alone."""
    torch, capi = g["torch"], g["capi"]
    win = rc.WINDOWS[wid][0]
    rows, cols = win[2:]
    out = cast(g, wid, workspace=True, signmap=True, pyramid=True)
    assert out["opts"].pyramid_built == 1
    r1, c1, r2, c2 = rows // 2, cols // 2, rows // 4, cols // 4
    ref = [DevMap(torch, 3 * r1, c1, c1 * 8 + 8), DevMap(torch, 3 * r1, c1, c1 * 8 + 8), DevMap(torch, 3 * r2, c2, c2 * 8 + 16), DevMap(torch, 3 * r2, c2, c2 * 8 + 16)]
    capi.resize_pyramid(out["vm"].addr, out["nm"].addr, out["vm"].pitch, rows, cols, ref[0].addr, ref[1].addr, ref[0].pitch, ref[2].addr, ref[3].addr, ref[2].pitch)
    torch.cuda.synchronize()
    n_valid = []
    for i, (got, want) in enumerate(zip(out["pyr"], ref)):
        r, c = (r1, c1) if i < 2 else (r2, c2)
        assert want.outside_untouched()
        if r == 0 or c == 0:
            assert got.untouched() and want.untouched(), (wid, i)
            continue
        n_valid.append(rc.assert_same_map(got.image(), want.image(), r, (wid, "level", 1 + i // 2, "normals" if i & 1 else "vertices")))
        assert under_sentinel_untouched(got, r), (wid, i)
        if wid in rc.PYRAMID_CROPS:
            rc.assert_same_map(got.image(), rc.crop(g["full"]["pyr"][i], win, level=1 + i // 2), r, (wid, "level", 1 + i // 2, "against the full frame's"))
    if wid in rc.PYRAMID_CROPS:
        assert min(n_valid) > 100, n_valid


@pytest.mark.parametrize("signmap", [False, True], ids=["full march", "sign map"])
@pytest.mark.parametrize("wid", IDS)
def test_slab_marches_composed(g, wid, signmap):
    """Three slabs (owned planes + a 6-plane halo, value / grad pointing at the first stored plane) composed (a) by masking and an
    integer sum of the maps and (b) by packing the owned pixels and scattering them: both are the crop of the full frame."""
    torch, capi, s, full = g["torch"], g["capi"], g["s"], g["full"]
    win = rc.WINDOWS[wid][0]
    y0, x0, rows, cols = win
    pitch = map_pitch(cols)
    kw = dict(signmap=g["sm"], signmap_shift=g["shift"], signmap_tranc_dist=s["trunc"]) if signmap else {}
    parts = []
    for owned in rc.OWNED:
        zs0, zs1 = rc.stored_of(owned)
        vm, nm, keys = DevMap(torch, 3 * rows, cols, pitch), DevMap(torch, 3 * rows, cols, pitch), DevFlat(torch, rows * cols, torch.int32)
        capi.raycast_slab(rc.window_intr(s["intr"], y0, x0), *s["pose"], s["trunc"], s["res"], s["vs"], g["value"][zs0 * N:], g["grad"][zs0 * N:],
                          N * 4, zs0, zs1, owned[0], owned[1], vm.addr, nm.addr, pitch, rows, cols, keys.t, **kw)
        parts.append((vm, nm, keys))
    torch.cuda.synchronize()
    for vm, nm, keys in parts:
        assert vm.outside_untouched() and nm.outside_untouched() and keys.outside_untouched(), (wid, "slab march")
    mk = parts[0][2].t.clone()
    for p in parts[1:]:
        mk = torch.minimum(mk, p[2].t)
    hkeys = np.stack([p[2].host() for p in parts])
    hmk, mine = rc.owners(hkeys)
    assert np.array_equal(hmk, mk.cpu().numpy())
    cv, cn = rc.crop(full["v"], win), rc.crop(full["n"], win)
    want_hits = int(rc.valid_of(cv, rows).sum())
    assert int(mine.sum()) == want_hits and (mine.sum(axis=0) <= 1).all()
    if wid in rc.TWO_OWNERS:
        assert int((mine.sum(axis=1) > 1000).sum()) >= 2, mine.sum(axis=1)
    # (b), first half: pack every slab's owned pixels into one entry buffer (before the mask touches the maps)
    entries, count = DevFlat(torch, rows * cols * rc.ENTRY_WORDS, torch.int32), torch.zeros(1, dtype=torch.int32, device="cuda")
    assert capi.raycast_compose_entry_bytes() == 4 * rc.ENTRY_WORDS
    for vm, nm, keys in parts:
        capi.raycast_compose_pack(keys.t, mk, vm.addr, nm.addr, pitch, rows, cols, entries.t, count)
    torch.cuda.synchronize()
    cnt = int(count.item())
    assert cnt == int(mine.sum())
    assert entries.outside_untouched() and entries.untouched_from(cnt * rc.ENTRY_WORDS)
    packed = entries.host()[:cnt * rc.ENTRY_WORDS].reshape(cnt, rc.ENTRY_WORDS)
    assert np.array_equal(np.sort(packed[:, 0]), np.flatnonzero(mine.any(axis=0)))
    # (a) mask, integer sum, finish
    sv, sn = DevMap(torch, 3 * rows, cols, pitch), DevMap(torch, 3 * rows, cols, pitch)
    sv.words.zero_(); sn.words.zero_()
    for vm, nm, keys in parts:
        capi.raycast_compose_mask(keys.t, mk, vm.addr, nm.addr, pitch, rows, cols)
        sv.words.add_(vm.words); sn.words.add_(nm.words)
    hits = torch.zeros(1, dtype=torch.int64, device="cuda")
    capi.raycast_compose_finish(mk, sv.addr, sn.addr, pitch, rows, cols, hits=hits)
    # (b), second half: scatter into zero-filled maps, finish
    bv, bn = DevMap(torch, 3 * rows, cols, pitch), DevMap(torch, 3 * rows, cols, pitch)
    bv.words.zero_(); bn.words.zero_()
    capi.raycast_compose_scatter(entries.t, cnt, bv.addr, bn.addr, pitch, rows, cols)
    hits_b = torch.zeros(1, dtype=torch.int64, device="cuda")
    capi.raycast_compose_finish(mk, bv.addr, bn.addr, pitch, rows, cols, hits=hits_b)
    torch.cuda.synchronize()
    for m in [sv, sn, bv, bn] + [p[0] for p in parts] + [p[1] for p in parts]:
        assert m.outside_untouched(), (wid, "composite")
    assert rc.assert_same_maps(sv.image(), sn.image(), cv, cn, rows, (wid, "mask + sum")) == want_hits == int(hits.item())
    assert rc.assert_same_maps(bv.image(), bn.image(), cv, cn, rows, (wid, "pack + scatter")) == want_hits == int(hits_b.item())


def test_sign_map_marches_without_the_short_division(g):
    """Everything above runs with voxel_size prepared (xs_const_div_prepare), i.e. the march instances that take floor(p / voxel_size)
    by the short division.  With it switched off the launchers pick the instances that divide — for the sign-map forms
    k_raycast<0, true, false, true> and <4, true, false, true>, which nothing else launches: windows A (ragged on both axes, one idle
    workgroup) and D (all workgroups busy, ragged lanes) through the fused sign-map launch and through three sign-map slab marches,
    composed, against the same crops of the full frame and with the same guards as above."""
    capi, vs = g["capi"], g["s"]["vs"]
    assert capi.const_div_state(vs) == 3
    was = capi.const_div_enable(0)
    try:
        assert capi.const_div_state(vs) == 0
        for wid in ("A", "D"):
            cast(g, wid, workspace=True, signmap=True)
            test_slab_marches_composed(g, wid, True)
    finally:
        capi.const_div_enable(was)
    assert capi.const_div_state(vs) == 3


@pytest.mark.parametrize("rows,cols", rc.COMPOSE_SHAPES)
def test_composite_kernels_on_crafted_keys(g, rows, cols):
    """mask, finish, pack and scatter against their numpy statements (raycast_cases.model_*), bit for bit, on keys of every kind and
    maps of random finite bit patterns; guards, and the entries beyond the count, untouched."""
    torch, capi = g["torch"], g["capi"]
    own, mn, kind = rc.crafted_keys(rows, cols, 100 * rows + cols)
    assert all((kind == k).sum() > 5 or rows * cols < 100 for k in range(6))
    hv, hn = rc.random_finite_map(rows, cols, 1), rc.random_finite_map(rows, cols, 2)
    assert not np.isnan(hv).any() and not np.isnan(hn).any()
    down = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    # behind either key array lie 256 keys of 0 (own == min, even: "mine"): a lane past the last pixel that looked at its keys would be counted
    d_own, d_mn = (down(np.concatenate([k, np.zeros(256, np.int32)]))[:rows * cols] for k in (own, mn))
    pitch = map_pitch(cols)

    def maps():
        v, n = DevMap(torch, 3 * rows, cols, pitch), DevMap(torch, 3 * rows, cols, pitch)
        v.words.copy_(down(hv.view(np.int32).reshape(3 * rows, 2 * cols))); n.words.copy_(down(hn.view(np.int32).reshape(3 * rows, 2 * cols)))
        return v, n

    def same(m, want, what):
        assert m.outside_untouched(), what
        assert np.array_equal(rc.planes_i32(m.image(), rows), want), what

    v, n = maps()
    capi.raycast_compose_mask(d_own, d_mn, v.addr, n.addr, pitch, rows, cols)
    torch.cuda.synchronize()
    same(v, rc.model_mask(own, mn, hv, rows), "mask, vertices"); same(n, rc.model_mask(own, mn, hn, rows), "mask, normals")

    v, n = maps()
    hits = torch.zeros(1, dtype=torch.int64, device="cuda")
    capi.raycast_compose_finish(d_mn, v.addr, n.addr, pitch, rows, cols, hits=hits)
    torch.cuda.synchronize()
    want_v, want_hits = rc.model_finish(mn, hv, rows)
    same(v, want_v, "finish, vertices"); same(n, rc.model_finish(mn, hn, rows)[0], "finish, normals")
    assert int(hits.item()) == want_hits and 0 < want_hits < rows * cols

    v, n = maps()
    entries, count = DevFlat(torch, rows * cols * rc.ENTRY_WORDS, torch.int32), torch.zeros(1, dtype=torch.int32, device="cuda")
    capi.raycast_compose_pack(d_own, d_mn, v.addr, n.addr, pitch, rows, cols, entries.t, count)
    torch.cuda.synchronize()
    want_e = rc.model_pack(own, mn, hv, hn, rows)
    cnt = int(count.item())
    assert cnt == len(want_e) and 0 < cnt < rows * cols
    assert entries.outside_untouched() and entries.untouched_from(cnt * rc.ENTRY_WORDS)
    got_e = entries.host()[:cnt * rc.ENTRY_WORDS].reshape(cnt, rc.ENTRY_WORDS)
    assert np.array_equal(got_e[np.argsort(got_e[:, 0], kind="stable")], want_e)
    same(v, rc.planes_i32(hv, rows), "pack leaves the maps alone"); same(n, rc.planes_i32(hn, rows), "pack leaves the maps alone")

    v, n = DevMap(torch, 3 * rows, cols, pitch), DevMap(torch, 3 * rows, cols, pitch)      # pattern-filled
    pv, pn = v.image().copy(), n.image().copy()
    capi.raycast_compose_scatter(entries.t, cnt, v.addr, n.addr, pitch, rows, cols)
    torch.cuda.synchronize()
    want_v, want_n = rc.model_scatter(got_e, pv, pn, rows)
    same(v, want_v, "scatter, vertices"); same(n, want_n, "scatter, normals")
    assert np.array_equal(want_v.reshape(3, -1, 2)[:, want_e[:, 0]], rc.planes_i32(hv, rows).reshape(3, -1, 2)[:, want_e[:, 0]])
