"""The cases that run the raycast (x-slam_amd/csrc/xs_raycast.hip) and its slab composite on ragged image windows.  A ray depends on
its pixel only through (x - cx) / fx and (y - cy) / fy; with a half-integer principal point and an integer origin (x0, y0),
float(x + x0) - cx and float(x) - (cx - x0) are the same float (both exact), so the raycast of a rows x cols window with intrinsics
(fx, fy, cx - x0, cy - y0) is the crop [y0 : y0 + rows, x0 : x0 + cols] of the full-frame raycast, bit for bit.  The full frame is held
against the oracle and the float64 model elsewhere (test_kernels_gpu.py, test_independent_gpu.py); here every launch form is held
against the crop, in guarded pitched buffers.  Backend-neutral parts first (tests/test_raycast_windows_cpu.py runs them on the oracle
alone), the device buffers and the numpy model of the composite kernels after them.  Test infrastructure."""
import functools

import numpy as np

from helpers import intr_of, s1_transforms, synth, tranc_dist
from map_cases import PATTERN

H, W = synth.HEIGHT, synth.WIDTH
N = 64                                        # volume edge (voxel size 0.12 m)
INT_MAX = 0x7FFFFFFF
SENTINEL = np.array([0x7FFFFFFF, 0], np.int32)   # (NaN, 0) as the kernels write it (xs_device.h: qnan_f)

# id -> ((y0, x0, rows, cols), pixels with a vertex in the oracle's raycast of that window).  With the default tiling (8 x 8 pixels a
# wave, 16 x 16 a workgroup, workgroups in multiples of 8):
#   A  ragged on both axes; 5 x 3 = 15 tiles, so 16 workgroups with 1 idle        B  the same, ending on the frame's last row and column
#   C  odd cols; 36 tiles, 40 workgroups with 4 idle; origin a multiple of 4      D  48 tiles, all busy, ragged lanes; origin a multiple of 4
#   E  one tile, 7 idle workgroups      F  one row      G  one column; 30 tiles, 32 workgroups with 2 idle      H  one pixel
WINDOWS = {
    "A": ((0, 0, 37, 70), 1035),
    "B": ((443, 570, 37, 70), 842),
    "C": ((96, 256, 50, 129), 4024),
    "D": ((60, 300, 122, 90), 9068),
    "E": ((232, 312, 16, 16), 256),
    "F": ((150, 0, 1, 640), 515),
    "G": ((0, 400, 480, 1), 406),
    "H": ((100, 380, 1, 1), 1),
}
PYRAMID_CROPS = ("C", "D")                    # origins that are multiples of 4: levels 1 and 2 are crops of the full frame's as well
TWO_OWNERS = ("C", "D")                       # two slabs own more than 1000 vertices each (oracle: 1419 / 2605 in C, 4751 / 4317 in D)
OWNED = [(0, 20), (20, 41), (41, 64)]         # z planes the three slabs own
HALO = 6


def stored_of(owned):
    return max(owned[0] - HALO, 0), min(owned[1] + HALO, N)


def window_intr(intr, y0, x0):
    """The intrinsics under which pixel (x, y) of a window casts the ray of pixel (x + x0, y + y0) of the frame."""
    k = np.asarray(intr, np.float32).copy()
    k[2], k[3] = k[2] - np.float32(x0), k[3] - np.float32(y0)
    assert float(k[2]) * 2 == int(float(k[2]) * 2) and float(k[3]) * 2 == int(float(k[3]) * 2)    # half-integers: exact
    return k


def crop(m, win, level=0):
    """[3 * h, w, c] (a map of the frame at a pyramid level, or [h, w] / [h * w] per-pixel values) -> the window's part."""
    y0, x0, rows, cols = win
    h, w = H >> level, W >> level
    y0, x0, rows, cols = y0 >> level, x0 >> level, rows >> level, cols >> level
    m = np.asarray(m)
    if m.ndim == 3:
        return np.ascontiguousarray(m.reshape(3, h, w, -1)[:, y0:y0 + rows, x0:x0 + cols]).reshape(3 * rows, cols, -1)
    return np.ascontiguousarray(m.reshape(h, w)[y0:y0 + rows, x0:x0 + cols])


def valid_of(m, rows):
    return ~np.isnan(np.asarray(m).reshape(3, rows, -1, 2)[0, ..., 0])


def assert_same_map(got, want, rows, what):
    """The comparison rule: the NaN-sentinel sets of plane 0 agree, and where a pixel is valid all three planes carry the same bits
    (under a sentinel the y / z planes hold whatever the buffer held).  Returns the number of valid pixels."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g, w = got.reshape(3, rows, -1, 2), want.reshape(3, rows, -1, 2)
    ok = valid_of(want, rows)
    assert np.array_equal(valid_of(got, rows), ok), (what, "sentinel sets differ", int((valid_of(got, rows) != ok).sum()))
    gb, wb = g.view(np.int32)[:, ok], w.view(np.int32)[:, ok]
    assert np.array_equal(gb, wb), (what, int((gb != wb).any(axis=(0, 2)).sum()), "valid pixels differ")
    return int(ok.sum())


def assert_same_maps(got_v, got_n, want_v, want_n, rows, what):
    hits = assert_same_map(got_v, want_v, rows, (what, "vertices"))
    assert_same_map(got_n, want_n, rows, (what, "normals"))
    return hits


@functools.lru_cache(maxsize=None)
def setting(oracle):
    """Scene S1 in a 64^3 volume built by the oracle from frames 0 and 1, rays from the pose of frame 2, and the oracle's full-frame
    raycast.  Computed once and shared: never modified."""
    prm = synth.s1_params(N)
    res = [N, N, N]
    v, w, g = oracle.new_volume(res)
    for k in (0, 1):
        T = s1_transforms(k, prm)
        oracle.integrate(oracle.scale_depth(synth.s1_frame(k)), v, w, g, res, tranc_dist(prm), 100, T["Rv2c"], T["tv2c"], intr_of(prm),
                         prm["tsdf_voxel_size"])
    T = s1_transforms(2, prm)
    s = dict(prm=prm, res=res, value=v, grad=g, T=T, intr=intr_of(prm), trunc=tranc_dist(prm), vs=prm["tsdf_voxel_size"])
    s["pose"] = (T["Rc2v"], T["tc2v"], T["Rv2w"], T["tv2w"])
    ov, on, ohits = oracle.raycast(s["intr"], *s["pose"], s["trunc"], res, s["vs"], v, g, H, W)
    for a in (v, g, ov, on):
        a.setflags(write=False)
    s.update(full_v=ov, full_n=on, full_hits=ohits)
    return s


def oracle_window(oracle, s, win):
    y0, x0, rows, cols = win
    return oracle.raycast(window_intr(s["intr"], y0, x0), *s["pose"], s["trunc"], s["res"], s["vs"], s["value"], s["grad"], rows, cols)


def oracle_slabs(oracle, s, win):
    """The three slab marches of a window on the oracle: [(vmap, nmap, keys)], and the reads outside the stored planes (must be 0)."""
    y0, x0, rows, cols = win
    parts, bad = [], 0
    for owned in OWNED:
        vm, nm, keys, b = oracle.raycast_slab(window_intr(s["intr"], y0, x0), *s["pose"], s["trunc"], s["res"], s["vs"], s["value"], s["grad"],
                                              rows, cols, stored_of(owned), owned)
        parts.append((vm, nm, keys))
        bad += b
    return parts, bad


def owners(keys):
    """keys: [slabs, pixels].  (min key, [slabs, pixels] does the slab hold the ray's first event and has that a vertex)."""
    keys = np.asarray(keys)
    mk = keys.min(axis=0)
    return mk, (keys == mk) & ((keys & 1) == 0) & (keys != INT_MAX)


def compose_numpy(parts, rows, cols):
    """The owner composite in plain numpy: the owner's vertex and normal, the sentinel where the first event has no vertex."""
    keys = np.stack([p[2] for p in parts])
    mk, mine = owners(keys)
    out = []
    for m in (0, 1):
        acc = np.zeros((3, rows, cols, 2), np.int32)
        for p, own in zip(parts, mine):
            acc += np.where(own.reshape(1, rows, cols, 1), np.asarray(p[m], np.float32).reshape(3, rows, cols, 2).view(np.int32), 0)
        acc[0][~mine.any(axis=0).reshape(rows, cols)] = SENTINEL
        out.append(acc.view(np.float32).reshape(3 * rows, cols, 2))
    return out[0], out[1], mk, mine


# ------------------------------------------------------------------------------------------------
# Device buffers with guards (torch tensors; torch is handed in by the GPU tests)
class DevMap:
    """rows x cols elements of elem bytes in (rows + 2) device rows of pitch bytes, one guard row before and one after, PATTERN
    everywhere.  addr: image row 0 (what a kernel is given)."""
    def __init__(self, torch, rows, cols, pitch, elem=8):
        assert pitch >= cols * elem and pitch % 4 == 0
        self.rows, self.cols, self.pitch, self.elem = rows, cols, int(pitch), elem
        self.buf = torch.full(((rows + 2) * self.pitch,), PATTERN, dtype=torch.uint8, device="cuda")
        self.addr = self.buf.data_ptr() + self.pitch
        # the image as int32 words on the device (for the composite's integer sum)
        self.words = self.buf.view(torch.int32).view(rows + 2, self.pitch // 4)[1:rows + 1, :cols * elem // 4]

    def host(self):
        return self.buf.cpu().numpy().reshape(self.rows + 2, self.pitch)

    def image(self):
        """float32 [rows, cols, 2] (a map of rows / 3 pixel rows: [3 * rows', cols, 2])"""
        return np.ascontiguousarray(self.host()[1:-1, :self.cols * self.elem]).view(np.float32).reshape(self.rows, self.cols, self.elem // 4)

    def outside_untouched(self):
        a = self.host()
        return bool((a[0] == PATTERN).all() and (a[-1] == PATTERN).all() and (a[1:-1, self.cols * self.elem:] == PATTERN).all())

    def untouched(self):
        return bool((self.host() == PATTERN).all())


class DevFlat:
    """n elements of a 4-byte dtype with GUARD elements before and after, PATTERN everywhere.  t: the n elements (a torch view)."""
    GUARD = 64

    def __init__(self, torch, n, dtype):
        self.n = n
        self.buf = torch.full(((n + 2 * self.GUARD) * 4,), PATTERN, dtype=torch.uint8, device="cuda").view(dtype)
        self.t = self.buf[self.GUARD:self.GUARD + n]

    def host(self):
        return self.t.cpu().numpy()

    def outside_untouched(self):
        a = self.buf.cpu().numpy().view(np.uint8)
        g = self.GUARD * 4
        return bool((a[:g] == PATTERN).all() and (a[g + self.n * 4:] == PATTERN).all())

    def untouched_from(self, first):
        """elements [first, n) still hold the pattern"""
        return bool((self.t[first:].cpu().numpy().view(np.uint8) == PATTERN).all())


def map_pitch(cols):
    return cols * 8 + 40


# ------------------------------------------------------------------------------------------------
# The composite kernels on crafted keys: inputs and a plain numpy statement of each kernel
COMPOSE_SHAPES = [(37, 70), (481, 641)]      # 481 x 641: 1205 pack blocks (the 1024-block stride and a ragged last block), 1331 finish tiles (the 256-block stride)
ENTRY_WORDS = 13


def crafted_keys(rows, cols, seed):
    """Per pixel one of: own == min and even | own == min and odd | own > min with min even | own > min with min odd | both INT_MAX |
    own INT_MAX with min finite.  Returns (own, min, kind)."""
    rng = np.random.default_rng(seed)
    n = rows * cols
    kind = rng.integers(0, 6, n)
    kind[:6] = np.arange(6)                                              # every kind at least once
    step = rng.integers(0, 17, n)
    odd = (kind == 1) | (kind == 3) | ((kind == 5) & (rng.random(n) < 0.5))
    mn = (step << 1) | odd
    own = mn.copy()
    more = (kind == 2) | (kind == 3)
    own[more] = mn[more] + rng.integers(1, 9, int(more.sum()))           # (either parity)
    own[kind >= 4] = INT_MAX
    mn[kind == 4] = INT_MAX
    return own.astype(np.int32), mn.astype(np.int32), kind


def random_finite_map(rows, cols, seed):
    """[3 * rows, cols, 2] float32 of random bit patterns, none of them NaN or infinite (denormals and both zeros included)."""
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 1 << 32, (3 * rows, cols, 2), dtype=np.uint64).astype(np.uint32)
    b[(b & 0x7F800000) == 0x7F800000] &= np.uint32(0xBFFFFFFF)
    return b.view(np.float32)


def planes_i32(m, rows):
    return np.asarray(m, np.float32).reshape(3, rows, -1, 2).view(np.int32)


def model_mask(own, mn, m, rows):
    """k_compose_mask: the map is kept where this rank holds the ray's first event and that has a vertex, zeroed elsewhere."""
    keep = ((own == mn) & ((own & 1) == 0) & (own != INT_MAX)).reshape(rows, -1)
    out = planes_i32(m, rows).copy()
    out[:, ~keep] = 0
    return out


def model_finish(mn, m, rows):
    """k_compose_finish: the sentinel in plane 0 where the first event has no vertex (odd key) or there is none; hits elsewhere."""
    none = (((mn & 1) == 1) | (mn == INT_MAX)).reshape(rows, -1)
    out = planes_i32(m, rows).copy()
    out[0][none] = SENTINEL
    return out, int((~none).sum())


def model_pack(own, mn, vm, nm, rows):
    """k_compose_pack: one 13-word entry per owned pixel with a vertex, here sorted by pixel index."""
    idx = np.flatnonzero((own == mn) & ((own & 1) == 0) & (own != INT_MAX))
    v, n = planes_i32(vm, rows).reshape(3, -1, 2), planes_i32(nm, rows).reshape(3, -1, 2)
    e = np.empty((idx.size, ENTRY_WORDS), np.int32)
    e[:, 0] = idx
    for q in range(3):
        e[:, 1 + 2 * q:3 + 2 * q] = v[q, idx]
        e[:, 7 + 2 * q:9 + 2 * q] = n[q, idx]
    return e


def model_scatter(entries, vm, nm, rows):
    """k_compose_scatter: every entry's six values written at its pixel, everything else left alone."""
    v, n = planes_i32(vm, rows).copy(), planes_i32(nm, rows).copy()
    cols = v.shape[2]
    y, x = entries[:, 0] // cols, entries[:, 0] % cols
    for q in range(3):
        v[q, y, x] = entries[:, 1 + 2 * q:3 + 2 * q]
        n[q, y, x] = entries[:, 7 + 2 * q:9 + 2 * q]
    return v, n
