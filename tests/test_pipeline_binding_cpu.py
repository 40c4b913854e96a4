"""CPU-only: what the Python binding (x-slam_amd/pipeline.py) hands to the C ABI and what it makes of the answer, with every entry
point replaced by a fake on the shared CDLL object.  No GPU and no volume: the instances are made without __init__ and carry a made-up
handle.  The fake checks every argument against the call's row of pl._SIGS, collects garbage (an argument array nobody holds any more
then shows as wrong contents), copies out the scalars and what lies behind the pointers, writes recognisable values into the outputs and
returns a scripted code.  Pinned per call: the C name, the leading arguments (handle; other.h or the encoded path; nothing), every scalar,
the arrays and their counts, the container, shape and dtype of what comes back, and the exception type and message per return code (the
strings are the binding's own, copied here as literals).  Host (numpy) arguments and outputs only."""
import ctypes as C
import gc
import importlib

import numpy as np
import pytest

pl = importlib.import_module("x-slam_amd.pipeline")
capi = importlib.import_module("x-slam_amd.capi")

H, H2, PATH = 0x51A0, 0x7B40, "/nowhere/map.xstsdf"
W = capi.FRONTIER_RECORD_WORDS
f32, f64, i32, u8, u16, u32, u64 = np.float32, np.float64, np.int32, np.uint8, np.uint16, np.uint32, np.uint64


def _address(a):
    if a is None or isinstance(a, int):
        return a
    if hasattr(a, "_obj"):                       # C.byref(x)
        return C.addressof(a._obj)
    if isinstance(a, (C.Array, C.Structure)):
        return C.addressof(a)
    return C.cast(a, C.c_void_p).value


def view(a, dtype, n):
    """The n items of dtype behind a pointer argument as a writable array, None for a null pointer."""
    p = _address(a)
    return None if p is None else np.frombuffer((C.c_char * (int(n) * np.dtype(dtype).itemsize)).from_address(p), dtype)


def rd(a, dtype, n):
    v = view(a, dtype, n)
    return None if v is None else v.copy()


def wr(a, dtype, n, base):
    """Writes base, base + 1, ... behind an output pointer (nothing for a null one) and returns what it wrote."""
    v = view(a, dtype, n)
    if v is None:
        return None
    v[:] = (np.arange(int(n)) + base).astype(dtype)
    return v.copy()


def fields(a):
    o = a._obj
    d = {k: getattr(o, k) for k, _ in o._fields_ if k != "user_T16xN"}
    if "user_n" in d:
        d["user"] = np.ctypeslib.as_array(o.user_T16xN, (d["user_n"] * 16,)).copy() if d["user_n"] else None
    return d


class Fakes:
    """Replaces entry points of pl._lib; calls holds (C name, what the decoder read) in call order."""

    def __init__(self, monkeypatch):
        self.mp, self.calls = monkeypatch, []

    def install(self, name, decode, codes, lead=0):
        codes, argtypes = list(codes), pl._SIGS[name][1]

        def fake(*args):
            assert len(args) == len(argtypes), name
            for t, a in zip(argtypes, args):
                t.from_param(a)
            gc.collect()
            churn = [np.full(k, 0x5A, u8) for k in (64, 128, 256, 512, 1024, 2048) for _ in range(4)]   # reuse what was freed
            rc = codes.pop(0) if len(codes) > 1 else codes[0]
            rec = decode(list(args[1 + lead:]), rc)
            rec.update(h=args[0], lead=list(args[1:1 + lead]), rc=rc)
            self.calls.append((name, rec))
            del churn
            return rc
        self.mp.setattr(pl._lib, name, fake)

    def names(self):
        return [n for n, _ in self.calls]


@pytest.fixture
def fakes(monkeypatch):
    return Fakes(monkeypatch)


def _instance(h):
    kf = object.__new__(pl.KinectFusion)
    kf.h, kf.res, kf.width, kf.height, kf.cfg = h, [8, 8, 8], 16, 12, {"tsdf_voxel_size": "0.01"}
    return kf


@pytest.fixture
def kf():
    a, b = _instance(H), _instance(H2)
    a.other = b
    yield a
    a.h = b.h = None


class Dev:
    """Stands in for a device depth image: only its address is asked for."""

    def data_ptr(self):
        return 0xD000


POSES = (np.arange(64, dtype=f32) * 0.25 - 3).reshape(2, 4, 4, 2)      # P = 2
POINTS = (np.arange(9, dtype=f32) * 0.5 + 1).reshape(3, 3)             # n = 3
TS = (np.arange(32, dtype=f64) - 7.5).reshape(2, 4, 4)                 # N = 2
T1 = np.arange(16, dtype=f64).reshape(4, 4) + 0.125
SEARCH_DEFAULTS = dict(box_t=0.31, refine_t=0.32)

# family -> (C name for the own map or None, another instance, a checkpoint) and the public methods in the same order
FAMILIES = {
    "merge": ((None, "xs_kf_merge_map", "xs_kf_merge_checkpoint"), (None, "merge_map", "merge_checkpoint")),
    "diff": ((None, "xs_kf_diff_map", "xs_kf_diff_checkpoint"), (None, "diff_map", "diff_checkpoint")),
    "align": ((None, "xs_kf_align_map", "xs_kf_align_checkpoint"), (None, "align_map", "align_checkpoint")),
    "align_global": ((None, "xs_kf_align_map_global", "xs_kf_align_checkpoint_global"), (None, "align_map_global", "align_checkpoint_global")),
    "score_transforms": ((None, "xs_kf_score_transforms", "xs_kf_score_transforms_checkpoint"), (None, "score_transforms", "score_transforms_checkpoint")),
    "render": (("xs_kf_render_views", "xs_kf_render_map", "xs_kf_render_checkpoint"), ("render_views", "render_map", "render_checkpoint")),
    "sample": (("xs_kf_sample_points", "xs_kf_sample_map", "xs_kf_sample_checkpoint"), ("sample", "sample_map", "sample_checkpoint")),
    "register": (("xs_kf_register_points", "xs_kf_register_map", "xs_kf_register_checkpoint"),
                 ("register_points", "register_map_points", "register_checkpoint_points")),
    "score_points": (("xs_kf_score_point_transforms", "xs_kf_score_point_transforms_map", "xs_kf_score_point_transforms_checkpoint"),
                     ("score_point_transforms", "score_map_point_transforms", "score_checkpoint_point_transforms")),
    "register_global": (("xs_kf_register_points_global", "xs_kf_register_points_global_map", "xs_kf_register_points_global_checkpoint"),
                        ("register_points_global", "register_map_points_global", "register_checkpoint_points_global")),
}
SOURCES = [(f, s) for f, (cn, _) in FAMILIES.items() for s in range(3) if cn[s] is not None]

# the part of the bad-arguments message that is the call's own
BAD = {
    "merge": "T not finite, min_weight < 1",
    "diff": "T, lo or hi not finite, lo > hi, min_weight < 1, a bad cell",
    "align": "T not finite, iterations < 0, min_weight < 1, max_residual or damping out of range",
    "align_global": "T not finite, a count, stride, box, min_weight, max_residual or damping out of range",
    "score_transforms": "T not finite, a count, stride, box, min_weight, max_residual or damping out of range",
    "render": "poses, intrinsics or size out of range or not finite, t_far <= t_near, more than 4096 samples, a map that cannot be rendered",
    "sample": "more than 2^30 points, T not finite, dvalue of a map without a grad array",
    "register": "more than 2^30 points, T not finite, iterations < 0, min_weight < 1, max_residual or damping out of range",
    "score_points": "more than 2^30 points, T not finite, a count, stride, box, min_weight, max_residual or damping out of range",
    "register_global": "more than 2^30 points or more than 2^24 scored ones (raise the stride), T not finite, a count, stride, box, min_weight, "
                       "max_residual or damping out of range",
}
ZERO_OK = {"align", "align_global", "register", "register_global"}


# ---- what each family's C call reads and writes (r: the arguments behind the handle and the source) ----

def d_merge(r, rc):
    view(r[2], u64, 1)[0] = 4242
    return dict(T=rd(r[0], f64, 16), min_weight=r[1])


def d_diff(r, rc):
    rec = dict(T=rd(r[0], f64, 16), min_weight=r[1], lo=r[2], hi=r[3], cell=r[4], min_size=r[5], capacity=r[6], masks=(r[12] is not None, r[13] is not None))
    n0, n1 = (37, 12) if rc == -4 else (5, 3)
    view(r[8], i32, 1)[0], view(r[10], i32, 1)[0] = n0, n1
    if rc == 1:
        rec["rec0"], rec["rec1"] = wr(r[7], u64, n0 * W, 1).reshape(-1, W), wr(r[9], u64, n1 * W, 1000).reshape(-1, W)
        view(r[11], u64, 3)[:] = (100, 7, 9)
        wr(r[12], u8, 512, 0), wr(r[13], u8, 512, 3)
    return rec


def d_align(r, rc):
    rec = dict(T=rd(r[0], f64, r[1] * 16), N=r[1], iterations=r[2], damping=r[3], min_weight=r[4], max_residual=r[5])
    if rc == 1:
        wr(r[6], f64, 16, 100), wr(r[8], f64, r[2] + 1, 0.5)
    view(r[7], f64, 8)[:] = (1, 50, 2.5, 0.05, 4, 1, 77, 0)
    return rec


def d_search(r, rc):
    rec = dict(opts=fields(r[0]))
    if rc == 1:
        wr(r[1], f64, 16, 200)
    wr(r[2], f64, 12, 1)
    return rec


def d_score_transforms(r, rc):
    wr(r[5], f64, 2 * r[0], 1)
    return dict(P=r[0], T=rd(r[1], f64, r[0] * 16), stride=r[2], min_weight=r[3], max_residual=r[4])


def d_render(r, rc):
    P, rows, cols = r[0], r[4], r[5]
    rec = dict(P=P, c2v=rd(r[1], f32, P * 16 * (2 if r[2] else 1)), is_complex=r[2], intr=rd(r[3], f32, 4), rows=rows, cols=cols, opts=fields(r[6]), on_device=r[12])
    n = P * rows * cols
    rec["wrote"] = dict(depth=wr(r[7], f32, n, 1), depth_u16=wr(r[8], u16, n, 2), normal=wr(r[9], f32, 3 * n, 3), shade=wr(r[10], u8, n, 4), counts=wr(r[11], u32, 4 * P, 5))
    return rec


def _sample_outputs(o, n_pix, base=0):
    return dict(status=wr(o[0], u8, n_pix, 1), value=wr(o[1], f32, n_pix, 2), dvalue=wr(o[2], f32, n_pix, 3), gradient=wr(o[3], f32, 3 * n_pix, 4), counts=wr(o[4], u64, 4, 5))


def d_sample(r, rc):
    return dict(n=r[0], points=rd(r[1], f32, r[0] * 3), T=rd(r[2], f64, 16), min_weight=r[3], flags=r[9], wrote=_sample_outputs(r[4:9], r[0]))


def d_register(r, rc):
    rec = dict(n=r[0], points=rd(r[1], f32, r[0] * 3), on_device=r[2], T=rd(r[3], f64, r[4] * 16), N=r[4], iterations=r[5], damping=r[6], min_weight=r[7],
               max_residual=r[8])
    if rc == 1:
        wr(r[9], f64, 16, 100), wr(r[11], f64, r[5] + 1, 0.5)
    view(r[10], f64, 7)[:] = (1, 50, 2.5, 0.05, 4, 1, 3)
    return rec


def d_score_points(r, rc):
    wr(r[8], f64, 2 * r[3], 1)
    return dict(n=r[0], points=rd(r[1], f32, r[0] * 3), on_device=r[2], P=r[3], T=rd(r[4], f64, r[3] * 16), stride=r[5], min_weight=r[6], max_residual=r[7])


def d_register_global(r, rc):
    rec = dict(n=r[0], points=rd(r[1], f32, r[0] * 3), on_device=r[2])
    rec.update(d_search(r[3:], rc))
    return rec


def d_defaults(r, rc):
    o = r[0]._obj
    o.struct_bytes, o.box_t, o.refine_t, o.user_n = C.sizeof(o), SEARCH_DEFAULTS["box_t"], SEARCH_DEFAULTS["refine_t"], 0
    return {}


DECODERS = {"merge": d_merge, "diff": d_diff, "align": d_align, "align_global": d_search, "score_transforms": d_score_transforms, "render": d_render,
            "sample": d_sample, "register": d_register, "score_points": d_score_points, "register_global": d_register_global}
SEARCH_KW = dict(candidates=64, keep=3, rounds=1, stride=2, refine_r=0.2, iterations=4, damping=2e-3, min_weight=2, max_residual=0.8)
# how each family's methods are called here, behind the source argument
CALLS = {
    "merge": ((T1,), dict(min_weight=2)),
    "diff": ((T1,), dict(min_weight=2, lo=-0.1, hi=0.4, cell_vox=8, min_size=3, masks=True, capacity=16)),
    "align": ((TS,), dict(iterations=3, damping=2e-3, min_weight=2, max_residual=0.8)),
    "align_global": ((), dict(SEARCH_KW, box_t=None, refine_t=0.07, Ts=TS)),
    "score_transforms": ((TS,), dict(stride=2, min_weight=2, max_residual=0.8)),
    "render": ((POSES,), dict(intr=(50.0, 51.0, 1.5, 1.0), size=(2, 3), t_near=0.3, t_far=4.0, step=0.02, min_weight=2,
                              outputs=("depth", "depth_u16", "normal", "shade", "counts"), cull=False)),
    "sample": ((POINTS,), dict(T=T1, min_weight=2, outputs=("status", "value", "dvalue", "gradient", "counts"))),
    "register": ((POINTS, TS), dict(iterations=3, damping=2e-3, min_weight=2, max_residual=0.8)),
    "score_points": ((POINTS, TS), dict(stride=2, min_weight=2, max_residual=0.8)),
    "register_global": ((POINTS,), dict(SEARCH_KW, box_t=0.5, refine_t=None, Ts=None)),
}


def install_family(fakes, family, codes):
    for s, cname in enumerate(FAMILIES[family][0]):
        if cname is not None:
            fakes.install(cname, DECODERS[family], codes, lead=int(s > 0))
    fakes.install("xs_kf_align_search_defaults", d_defaults, [0])
    fakes.install("xs_kf_register_search_defaults", d_defaults, [0])


def call_family(kf, family, s, args=None, **over):
    a, kw = CALLS[family]
    src = ((), (kf.other,), (PATH,))[s]
    return getattr(kf, FAMILIES[family][1][s])(*src, *(a if args is None else args), **dict(kw, **over))


def family_calls(fakes):
    return [(n, r) for n, r in fakes.calls if not n.endswith("_search_defaults")]


def check_search_opts(o, box_t, refine_t, user):
    assert o["struct_bytes"] == C.sizeof(pl.AlignSearchOpts) == C.sizeof(pl.RegisterSearchOpts)
    assert (o["candidates"], o["keep"], o["rounds"], o["stride"], o["iterations"], o["min_weight"]) == (64, 3, 1, 2, 4, 2)
    assert (o["box_t"], o["refine_t"], o["refine_r"], o["damping"], o["max_residual"]) == (box_t, refine_t, 0.2, 2e-3, 0.8)
    if user is None:
        assert o["user_n"] == 0 and o["user"] is None
    else:
        assert o["user_n"] == 2 and np.array_equal(o["user"], user.reshape(-1))


@pytest.mark.parametrize("family,s", SOURCES)
def test_source_taking_methods_pass_and_return_what_is_documented(kf, fakes, family, s):
    install_family(fakes, family, [1])
    out = call_family(kf, family, s)
    (name, r), = family_calls(fakes)
    assert name == FAMILIES[family][0][s]
    assert r["h"] == H and r["lead"] == [[], [H2], [PATH.encode()]][s]
    if family == "merge":
        assert np.array_equal(r["T"], T1.reshape(-1)) and r["min_weight"] == 2 and out == 4242 and type(out) is int
    elif family == "diff":
        assert np.array_equal(r["T"], T1.reshape(-1)) and (r["min_weight"], r["lo"], r["hi"], r["cell"], r["min_size"], r["capacity"]) == (2, -0.1, 0.4, 8, 3, 16)
        assert r["masks"] == (True, True) and isinstance(out, pl.MapDiff) and out.counts == dict(compared=100, only_this=7, only_other=9)
        for got, rec, n in ((out.only_this, r["rec0"], 5), (out.only_other, r["rec1"], 3)):
            assert got.dtype == pl.KinectFusion.FRONTIER_DTYPE and got.shape == (n,)
            assert np.array_equal(got["label"], rec[:, 0]) and np.array_equal(got["count"], rec[:, 1]) and np.array_equal(got["sum"], rec[:, 2:5])
        assert all(m.dtype == u8 and m.shape == (8, 8, 8) for m in out.masks)
        assert np.array_equal(out.masks[0].reshape(-1), np.arange(512).astype(u8)) and out.masks[1].reshape(-1)[0] == 3
    elif family in ("align", "register"):
        assert np.array_equal(r["T"], TS.reshape(-1)) and (r["N"], r["iterations"], r["damping"], r["min_weight"], r["max_residual"]) == (2, 3, 2e-3, 2, 0.8)
        ok, T, rep = out[:3]
        assert ok is True and T.dtype == f64 and np.array_equal(T, np.arange(16.0).reshape(4, 4) + 100)
        hist = out[3] if family == "align" else rep.pop("loss_history")
        assert hist.dtype == f64 and np.array_equal(hist, np.arange(4) + 0.5)
        last = dict(band_voxels=77) if family == "align" else dict(points=3)
        assert rep == dict(start=1, count=50, sum_r2=2.5, loss=0.05, passes=4, ended_ok=1, **last) and len(out) == (4 if family == "align" else 3)
    elif family in ("align_global", "register_global"):
        if family == "align_global":
            check_search_opts(r["opts"], SEARCH_DEFAULTS["box_t"], 0.07, TS)
        else:
            check_search_opts(r["opts"], 0.5, SEARCH_DEFAULTS["refine_t"], None)
        ok, T, rep = out
        assert ok is True and T.dtype == f64 and np.array_equal(T, np.arange(16.0).reshape(4, 4) + 200)
        names = ("band_voxels", "scored_entries") if family == "align_global" else ("points", "scored_points")
        assert rep == {"rank": 1, "S_before": 2.0, "count": 3, "sum_r2": 4.0, "loss": 5.0, "score_launches": 6, "passes": 7, "ended_ok": 8, names[0]: 9,
                       names[1]: 10, "centroid_distance": 11.0}
        assert all(type(rep[k]) is (float if k in ("S_before", "sum_r2", "loss", "centroid_distance") else int) for k in rep)
    elif family in ("score_transforms", "score_points"):
        assert r["P"] == 2 and np.array_equal(r["T"], TS.reshape(-1)) and (r["stride"], r["min_weight"], r["max_residual"]) == (2, 2, 0.8)
        assert isinstance(out, np.ndarray) and out.dtype == f64 and np.array_equal(out, np.arange(1.0, 5.0).reshape(2, 2))
    elif family == "render":
        assert (r["P"], r["is_complex"], r["rows"], r["cols"], r["on_device"]) == (2, 1, 2, 3, 0) and np.array_equal(r["c2v"], POSES.reshape(-1))
        assert np.array_equal(r["intr"], np.array([50, 51, 1.5, 1], f32))
        assert r["opts"] == dict(struct_bytes=C.sizeof(capi.RenderOpts), t_near=f32(0.3), t_far=4.0, step=f32(0.02), min_weight=2, cull=0, shade_mode=0)
        assert isinstance(out, pl.RenderedViews)
        want = dict(depth=((2, 2, 3), f32), depth_u16=((2, 2, 3), u16), normal=((2, 3, 2, 3), f32), shade=((2, 2, 3), u8), counts=((2, 4), u32))
        for k, (shape, dt) in want.items():
            got = getattr(out, k)
            assert type(got) is np.ndarray and got.shape == shape and got.dtype == dt and np.array_equal(got.reshape(-1), r["wrote"][k]), k
    elif family == "sample":
        assert r["n"] == 3 and np.array_equal(r["T"], T1.reshape(-1)) and (r["min_weight"], r["flags"]) == (2, 0) and isinstance(out, pl.MapSamples)
        want = dict(status=((3,), u8), value=((3,), f32), dvalue=((3,), f32), gradient=((3, 3), f32), counts=((4,), u64))
        for k, (shape, dt) in want.items():
            got = getattr(out, k)
            assert type(got) is np.ndarray and got.shape == shape and got.dtype == dt and np.array_equal(got.reshape(-1), r["wrote"][k]), k
    if "points" in r:
        assert r["n"] == 3 and np.array_equal(r["points"], POINTS.reshape(-1)) and r.get("on_device", 0) == 0


def test_defaults_and_optional_arguments(kf, fakes):
    """What the methods pass when the caller leaves an argument out: the identity for T, null pointers for an absent T or intrinsics, only the
    outputs asked for, render_map's and render_checkpoint's defaults equal to render_views', a real pose stack."""
    for family in ("merge", "diff", "align", "render", "sample", "register"):
        install_family(fakes, family, [1])
    kf.merge_map(kf.other)
    kf.diff_checkpoint(PATH)
    kf.align_map(kf.other)
    kf.register_points(POINTS)
    eye = np.eye(4).reshape(-1)
    merge, diff, align, reg = (r for _, r in fakes.calls)
    assert np.array_equal(merge["T"], eye) and merge["min_weight"] == 1
    assert np.array_equal(diff["T"], eye) and (diff["min_weight"], diff["lo"], diff["hi"], diff["cell"], diff["min_size"], diff["capacity"]) == (1, 0.0, 0.5, 0, 8, 1024)
    assert diff["masks"] == (False, False)
    assert np.array_equal(align["T"], eye) and (align["N"], align["iterations"], align["damping"], align["min_weight"], align["max_residual"]) == (1, 10, 1e-3, 1, 1.0)
    assert np.array_equal(reg["T"], eye) and (reg["N"], reg["iterations"], reg["max_residual"]) == (1, 10, 0.9)
    del fakes.calls[:]
    views = [kf.render_views(POSES[..., 0]), kf.render_map(kf.other, POSES[..., 0]), kf.render_checkpoint(PATH, POSES[..., 0])]
    for (_, r), v in zip(fakes.calls, views):
        assert (r["P"], r["is_complex"], r["rows"], r["cols"]) == (2, 0, 12, 16) and r["intr"] is None and np.array_equal(r["c2v"], POSES[..., 0].reshape(-1))
        assert r["opts"] == dict(struct_bytes=C.sizeof(capi.RenderOpts), t_near=f32(0.2), t_far=5.0, step=0.0, min_weight=1, cull=1, shade_mode=0)
        assert [k for k in v._fields if getattr(v, k) is not None] == ["depth", "normal", "shade"] and r["wrote"]["counts"] is None and r["wrote"]["depth_u16"] is None
    del fakes.calls[:]
    one = kf.render_map(kf.other, POSES[0], outputs=("counts",))            # a single pose [4, 4, 2], options through **kw
    assert fakes.calls[0][1]["P"] == 1 and one.counts.shape == (1, 4) and one.depth is None
    del fakes.calls[:]
    s = kf.sample(POINTS)
    r = fakes.calls[0][1]
    assert r["T"] is None and r["min_weight"] == 1 and [k for k in s._fields if getattr(s, k) is not None] == ["status", "value", "gradient"]
    assert r["wrote"]["dvalue"] is None and r["wrote"]["counts"] is None


@pytest.mark.parametrize("family,s", SOURCES)
@pytest.mark.parametrize("rc", [0, -1, -2, -3, -7])
def test_source_taking_methods_map_the_return_code(kf, fakes, family, s, rc):
    install_family(fakes, family, [rc])
    name = FAMILIES[family][0][s]
    if rc == 0 and family in ZERO_OK:
        out = call_family(kf, family, s)
        assert out[0] is False
        if family in ("align", "register"):
            assert np.array_equal(out[1], TS[0]) and len(out[3] if family == "align" else out[2]["loss_history"]) == 0
        else:
            assert np.array_equal(out[1], np.eye(4))
        return
    kind, text = {0: (ValueError, f"{name}: no volume"), -2: (capi.XsError, f"{name}: not available in shard mode"),
                  -1: (ValueError, f"{name}: bad arguments ({BAD[family]}, the volume itself as source, a bad file or another truncation distance)")}.get(
                      rc, (ValueError, f"{name}: {rc}"))
    with pytest.raises(kind) as e:
        call_family(kf, family, s)
    assert type(e.value) is kind and str(e.value) == text
    assert [n for n, _ in family_calls(fakes)] == [name]


# ---- the calls that take no second map ----

def d_views(r, rc):      # score_views / next_best_view / next_reachable_view / next_view_by_travel: P, poses, opts, min_weight, [min_hits,] out, ...
    rec = dict(P=r[0], poses=rd(r[1], f32, r[0] * 32), opts=fields(r[2]), min_weight=r[3])
    rest = r[4:]
    if not isinstance(rest[0], int):
        wr(rest[0], u32, 4 * r[0], 1)
        return rec
    rec["min_hits"] = rest[0]
    wr(rest[1], u32, 4 * r[0], 1)
    rec["tail"] = [x for x in rest[2:] if isinstance(x, (int, float))]
    if len(rest) == 6:
        wr(rest[5], u8, r[0], 1)                     # next_reachable_view's flags
    if len(rest) == 8:
        view(rest[7], u16, r[0])[:] = (6, 65535)     # next_view_by_travel's costs
    return rec


def d_clearance(r, rc):
    wr(r[3], u16, 512, 7)
    return dict(scalars=r[:3])


def d_reach(r, rc):      # reachable / travel
    k = int(len(r) == 11)       # travel carries max_travel_m and a cost array
    P = r[5 + k]
    wr(r[7 + k], u8, P, 0), wr(r[8 + k], u16, P, 20)
    if k:
        view(r[10], u16, P)[:] = (6, 65535)
    return dict(start=rd(r[0], f32, 32), scalars=r[1:5 + k], P=P, poses=rd(r[6 + k], f32, P * 32))


def d_path(r, rc):
    n = 37 if rc == -4 else max(rc, 0)
    view(r[10], i32, 1)[0] = n
    if rc > 0:
        wr(r[8], i32, 3 * rc, 1), wr(r[9], f32, 3 * rc, 0.5)
    return dict(start=rd(r[0], f32, 32), scalars=r[1:6], target=rd(r[6], f32, 32), capacity=r[7])


def d_frontiers(r, rc):
    n = 37 if rc == -4 else 5
    view(r[5], i32, 1)[0] = n
    return dict(scalars=r[:3], capacity=r[3], rec=wr(r[4], u64, n * W, 1).reshape(-1, W) if rc == 1 else None)


def d_propose(r, rc):
    n = 37 if rc == -4 else 5
    view(r[12], i32, 1)[0] = n
    if rc == 1:
        wr(r[10], f32, 32 * n, 1), wr(r[11], i32, n, 9)
    return dict(scalars=r[:9], capacity=r[9])


def d_reintegrate(r, rc):
    n = r[0]
    view(r[7], u64, 4)[:] = (11, 12, 13, 14)
    return dict(n=n, depths=list(r[1]), step=r[2], olds=rd(r[3], f32, 32 * n), news=rd(r[4], f32, 32 * n), modes=rd(r[5], i32, n), frames=rd(r[6], i32, n))


def d_fuse(r, rc):
    view(r[9], u64, 5)[:] = (21, 22, 23, 24, 25)
    return dict(n=r[0], points=rd(r[1], f32, 3 * r[0]), on_device=r[2], T=rd(r[3], f64, 16), origin=rd(r[4], f32, 3), scalars=r[5:9])


def d_score_poses(r, rc):
    wr(r[4], f64, 2 * r[2], 1)
    return dict(depth=r[0], step=r[1], P=r[2], poses=rd(r[3], f32, 32 * r[2]))


def d_reloc_global(r, rc):
    if rc == 1:
        wr(r[7], f32, 32, 300)
    view(r[8], f64, 8)[:] = (1, 2.5, 3.5, 4.5, 5, 1, 99, 0)
    return dict(depth=r[0], step=r[1], P=r[2], poses=rd(r[3], f32, 32 * r[2]), scalars=r[4:7])


def d_residuals(r, rc):
    rows, cols = r[5], r[6]
    return dict(depth=rd(r[0], u16, rows * cols), step=r[1], c2v=rd(r[2], f32, 32 if r[3] else 16), is_complex=r[3], intr=rd(r[4], f32, 4), rows=rows, cols=cols,
                min_weight=r[7], flags=r[13], wrote=_sample_outputs(r[8:13], rows * cols))


VIEW, REACH, FRONT = ("occlusion along a ray is not additive over z-slabs", "distance and connectivity are not additive over z-slabs",
                      "neither connectivity nor a cluster is additive over z-slabs")
# method -> (C name, decoder, how it is called, its shard-mode reason, {return code: (exception type, message)}, the codes that are results)
PLAIN = {
    "score_views": ("xs_kf_score_views", d_views, lambda k: k.score_views(POSES), VIEW, {0: "no volume", -1: "bad arguments or options", -3: "no volume", -7: "no volume"}, ()),
    "next_best_view": ("xs_kf_next_best_view", d_views, lambda k: k.next_best_view(POSES), VIEW, {-3: "bad arguments or options"}, (0, -1, -7)),
    "next_reachable_view": ("xs_kf_next_reachable_view", d_views, lambda k: k.next_reachable_view(POSES, 0.2), REACH, {-3: "bad arguments or options"}, (0, -1, -7)),
    "next_view_by_travel": ("xs_kf_next_view_by_travel", d_views, lambda k: k.next_view_by_travel(POSES, 0.2), REACH, {-3: "bad arguments or options"}, (0, -1, -7)),
    "clearance_field": ("xs_kf_clearance_field", d_clearance, lambda k: k.clearance_field(), REACH,
                        {0: "no volume", -1: "bad arguments or options", -3: "no volume", -7: "no volume"}, ()),
    "reachable": ("xs_kf_reachable", d_reach, lambda k: k.reachable(POSES, 0.2), REACH, {0: "no volume", -1: "bad arguments or options", -3: "no volume", -7: "no volume"}, ()),
    "travel": ("xs_kf_travel", d_reach, lambda k: k.travel(POSES, 0.2), REACH, {0: "no volume", -1: "bad arguments or options", -3: "no volume", -7: "no volume"}, ()),
    "path_to": ("xs_kf_path_to", d_path, lambda k: k.path_to(POSES[0], 0.2), REACH, {-1: "bad arguments or options", -3: (capi.XsError, "-3"), -7: (capi.XsError, "-7")}, (0,)),
    "frontiers": ("xs_kf_frontiers", d_frontiers, lambda k: k.frontiers(), FRONT, {0: "no volume", -1: "bad arguments or options", -3: "-3", -7: "-7"}, ()),
    "propose_views": ("xs_kf_propose_views", d_propose, lambda k: k.propose_views(0.2), FRONT, {0: "no volume", -1: "bad arguments or options", -3: "-3", -7: "-7"}, ()),
    "score_poses": ("xs_kf_score_poses", d_score_poses, lambda k: k.score_poses(Dev(), POSES), None,
                    {0: "no volume", -1: "bad arguments", -2: "bad arguments", -3: "bad arguments", -7: "bad arguments"}, ()),
    "relocalize_global": ("xs_kf_relocalize_global", d_reloc_global, lambda k: k.relocalize_global(Dev(), POSES), None,
                          {-1: "bad arguments", -2: "bad arguments", -3: "bad arguments", -7: "bad arguments"}, (0,)),
}


@pytest.mark.parametrize("method", sorted(PLAIN))
@pytest.mark.parametrize("rc", [0, -1, -2, -3, -7])
def test_plain_methods_map_the_return_code(kf, fakes, method, rc):
    name, decode, call, reason, raises, results = PLAIN[method]
    fakes.install(name, decode, [rc])
    if rc in results:
        out = call(kf)
        if method == "path_to":
            assert out is None
        elif method == "relocalize_global":
            assert out[0] is False and np.array_equal(out[1], POSES[0]) and out[2]["index"] == 1
        else:
            assert out[0] == rc and type(out[0]) is int
        return
    if rc == -2 and reason is not None:
        kind, text = capi.XsError, f"{name}: not available in shard mode ({reason})"
    else:
        kind, text = raises[rc] if isinstance(raises[rc], tuple) else (ValueError, raises[rc])
        text = f"{name}: {text}"
    with pytest.raises(kind) as e:
        call(kf)
    assert type(e.value) is kind and str(e.value) == text and fakes.names() == [name]


def test_plain_methods_pass_and_return_what_is_documented(kf, fakes):
    for method, (name, decode, _, _, _, _) in PLAIN.items():
        fakes.install(name, decode, [3] if method in ("next_best_view", "next_reachable_view", "next_view_by_travel", "path_to") else [1])
    start = POSES[1] + 1
    poses, vopts = POSES.reshape(-1), dict(struct_bytes=C.sizeof(capi.ViewOpts), rays_x=8, rays_y=6, t_near=f32(0.3), t_far=4.0, step=0.0)
    counts = np.arange(1, 9, dtype=u32).reshape(2, 4)
    vkw = dict(rays=(8, 6), t_near=0.3, t_far=4.0, min_weight=2)

    out = kf.score_views(POSES, **vkw)
    r = fakes.calls.pop()[1]
    assert r["h"] == H and r["P"] == 2 and np.array_equal(r["poses"], poses) and r["opts"] == vopts and r["min_weight"] == 2
    assert type(out) is np.ndarray and out.dtype == u32 and np.array_equal(out, counts)

    idx, out = kf.next_best_view(POSES, **vkw)
    r = fakes.calls.pop()[1]
    assert idx == 3 and r["P"] == 2 and np.array_equal(r["poses"], poses) and r["opts"] == vopts and (r["min_weight"], r["min_hits"]) == (2, 12) and np.array_equal(out, counts)

    idx, out, flags = kf.next_reachable_view(POSES, 0.25, min_hits=5, snap_vox=3, unknown_blocks=False, **vkw)
    r = fakes.calls.pop()[1]
    assert idx == 3 and r["min_hits"] == 5 and r["tail"] == [0.25, 3, 0] and np.array_equal(out, counts) and flags.dtype == bool and flags.tolist() == [True, True]

    idx, out, travel_m = kf.next_view_by_travel(POSES, 0.25, bias_m=0.75, max_travel_m=9.0, **vkw)
    r = fakes.calls.pop()[1]
    assert idx == 3 and r["min_hits"] == 12 and r["tail"] == [0.25, 4, 1, 9.0, 0.75] and np.array_equal(out, counts)
    vs = float(f32(0.01))
    assert travel_m.dtype == f64 and travel_m[0] == 6 * vs / 3.0 and travel_m[1] == np.inf

    out = kf.clearance_field(max_radius_vox=5, unknown_blocks=False, min_weight=2)
    r = fakes.calls.pop()[1]
    assert r["scalars"] == [5, 0, 2] and out.dtype == u16 and out.shape == (8, 8, 8) and np.array_equal(out.reshape(-1), np.arange(512) + 7)

    flags, clear2 = kf.reachable(POSES, 0.25, start=start, snap_vox=3, unknown_blocks=False, min_weight=2)
    r = fakes.calls.pop()[1]
    assert np.array_equal(r["start"], start.reshape(-1)) and r["scalars"] == [0.25, 3, 0, 2] and r["P"] == 2 and np.array_equal(r["poses"], poses)
    assert flags.dtype == bool and flags.tolist() == [False, True] and clear2.dtype == u16 and clear2.tolist() == [20, 21]

    flags, clear2, travel_m = kf.travel(POSES, 0.25)
    r = fakes.calls.pop()[1]
    assert r["start"] is None and r["scalars"] == [0.25, 4, 1, 1, 0.0] and r["P"] == 2 and np.array_equal(r["poses"], poses)
    assert flags.tolist() == [False, True] and clear2.tolist() == [20, 21] and travel_m[0] == 6 * vs / 3.0 and travel_m[1] == np.inf

    points, voxels = kf.path_to(POSES[1], 0.25, start=start, max_travel_m=9.0, capacity=8)
    r = fakes.calls.pop()[1]
    assert np.array_equal(r["start"], start.reshape(-1)) and r["scalars"] == [0.25, 4, 1, 1, 9.0] and np.array_equal(r["target"], POSES[1].reshape(-1)) and r["capacity"] == 8
    assert points.dtype == f32 and points.shape == (3, 3) and points[0, 0] == 0.5 and voxels.dtype == i32 and np.array_equal(voxels, np.arange(1, 10).reshape(3, 3))

    out = kf.frontiers(cell_vox=8, min_size=3, min_weight=2)
    r = fakes.calls.pop()[1]
    assert r["scalars"] == [8, 3, 2] and r["capacity"] == 1024 and out.dtype == pl.KinectFusion.FRONTIER_DTYPE and out.shape == (5,)
    assert np.array_equal(out["label"], r["rec"][:, 0]) and np.array_equal(out["count"], r["rec"][:, 1])

    c2vs, cluster = kf.propose_views(0.25, views_per_cluster=4, standoff_m=0.8, cell_vox=8, min_size=3, snap_vox=2, start_snap_vox=5, unknown_blocks=False, min_weight=2)
    r = fakes.calls.pop()[1]
    assert r["scalars"] == [0.25, 5, 0, 2, 8, 3, 4, 0.8, 2] and r["capacity"] == 1024
    assert c2vs.dtype == f32 and c2vs.shape == (5, 4, 4, 2) and c2vs.reshape(-1)[0] == 1 and cluster.dtype == i32 and cluster.tolist() == [9, 10, 11, 12, 13]

    loss, count = kf.score_poses(Dev(), POSES)
    r = fakes.calls.pop()[1]
    assert (r["depth"], r["step"], r["P"]) == (0xD000, 32, 2) and np.array_equal(r["poses"], poses) and loss.tolist() == [1.0, 3.0] and count.tolist() == [2.0, 4.0]

    ok, best, rep = kf.relocalize_global(Dev(), POSES, keep=3, iterations=4, damping=2e-3)
    r = fakes.calls.pop()[1]
    assert (r["depth"], r["step"], r["P"]) == (0xD000, 32, 2) and np.array_equal(r["poses"], poses) and r["scalars"] == [3, 4, 2e-3]
    assert ok is True and best.shape == (4, 4, 2) and best.reshape(-1)[0] == 300
    assert rep == dict(index=1, S_before=2.5, S_after=3.5, sum_loss_after=4.5, count_after=5.0, refined_ok=1, index_voxels=99)
    assert fakes.calls == []


@pytest.mark.parametrize("rc", [1, 0, -1, -2, -3, -7])
def test_reintegrate_and_fuse_points(kf, fakes, rc):
    fakes.install("xs_kf_reintegrate", d_reintegrate, [rc])
    fakes.install("xs_kf_fuse_points", d_fuse, [rc])
    olds, news = POSES, POSES + 1
    calls = (lambda: kf.reintegrate_batch([0xD000, 0xD100], olds, news, frames=[4, None]),
             lambda: kf.fuse_points(POINTS, T1, origin=(0.5, 0.25, 2.0), min_range=0.3, max_range=4.0, carve=True, weight=2))
    if rc == 1:
        assert calls[0]() == dict(removed=11, added=12, emptied=13, orphaned=14)
        assert calls[1]() == dict(used=21, dropped=22, visits=23, outside=24, written=25)
        (_, a), (_, b) = fakes.calls
        assert (a["n"], a["depths"], a["step"]) == (2, [0xD000, 0xD100], 32) and np.array_equal(a["olds"], olds.reshape(-1)) and np.array_equal(a["news"], news.reshape(-1))
        assert a["modes"].tolist() == [3, 3] and a["frames"].tolist() == [4, -1]
        assert (b["n"], b["on_device"]) == (3, 0) and np.array_equal(b["points"], POINTS.reshape(-1)) and np.array_equal(b["T"], T1.reshape(-1))
        assert b["origin"].tolist() == [0.5, 0.25, 2.0] and b["scalars"] == [0.3, 4.0, 1, 2]
        del fakes.calls[:]
        kf.deintegrate(Dev(), POSES[0])
        kf.fuse_points(POINTS)
        (_, a), (_, b) = fakes.calls
        assert a["n"] == 1 and a["news"] is None and a["frames"] is None and a["modes"].tolist() == [1] and b["T"] is None and b["origin"].tolist() == [0, 0, 0]
        return
    fuse = "xs_kf_fuse_points"
    bad = "T, origin or a range not finite, min_range <= 0, max_range < min_range or too long, weight outside 1 .. max_integration_weight"
    want = ({0: (ValueError, "reintegrate: no volume"), -2: (capi.XsError, "reintegrate: not available in shard mode")}.get(
                rc, (ValueError, "reintegrate: bad arguments (a pose that is not finite, a frame index past the record)")),
            {0: (ValueError, f"{fuse}: no volume"), -2: (capi.XsError, f"{fuse}: not available in shard mode"),
             -1: (ValueError, f"{fuse}: bad arguments ({bad}, the volume itself as source, a bad file or another truncation distance)")}.get(
                rc, (ValueError, f"{fuse}: {rc}")))
    for call, (kind, text) in zip(calls, want):
        with pytest.raises(kind) as e:
            call()
        assert type(e.value) is kind and str(e.value) == text


def test_frame_residuals(kf, fakes):
    fakes.install("xs_kf_frame_residuals", d_residuals, [1])
    depth = np.arange(6, dtype=u16).reshape(2, 3) + 400
    out = kf.frame_residuals(depth, POSES[0], min_weight=2, outputs=("status", "value", "dvalue", "gradient", "counts"), intr=(50.0, 51.0, 1.5, 1.0))
    (_, r), = fakes.calls
    assert np.array_equal(r["depth"], depth.reshape(-1)) and (r["step"], r["is_complex"], r["rows"], r["cols"], r["min_weight"], r["flags"]) == (6, 1, 2, 3, 2, 0)
    assert np.array_equal(r["c2v"], POSES[0].reshape(-1)) and r["intr"].tolist() == [50.0, 51.0, 1.5, 1.0] and isinstance(out, pl.FrameResiduals)
    want = dict(status=((2, 3), u8), value=((2, 3), f32), dvalue=((2, 3), f32), gradient=((3, 2, 3), f32), counts=((4,), u64))
    for k, (shape, dt) in want.items():
        got = getattr(out, k)
        assert type(got) is np.ndarray and got.shape == shape and got.dtype == dt and np.array_equal(got.reshape(-1), r["wrote"][k]), k
    del fakes.calls[:]
    out = kf.frame_residuals(depth, POSES[0, ..., 0])
    r = fakes.calls[0][1]
    assert r["is_complex"] == 0 and r["intr"] is None and [k for k in out._fields if getattr(out, k) is not None] == ["status", "value"]
    fakes.install("xs_kf_frame_residuals", d_residuals, [-1])
    with pytest.raises(ValueError) as e:
        kf.frame_residuals(depth, POSES[0])
    assert str(e.value) == ("xs_kf_frame_residuals: bad arguments (an empty or oversized image, a pose or intrinsics that are not finite, the volume itself as source, "
                            "a bad file or another truncation distance)")


def test_malformed_arguments_raise_before_any_c_call(kf, fakes):
    for family in FAMILIES:
        install_family(fakes, family, [1])
    for method, (name, decode, _, _, _, _) in PLAIN.items():
        fakes.install(name, decode, [1])
    fakes.install("xs_kf_fuse_points", d_fuse, [1])
    fakes.install("xs_kf_frame_residuals", d_residuals, [1])
    short = np.zeros(31, f32)
    for call in (lambda: kf.score_views(short), lambda: kf.next_best_view(short), lambda: kf.reachable(short, 0.2), lambda: kf.travel(short, 0.2),
                 lambda: kf.next_reachable_view(short, 0.2), lambda: kf.next_view_by_travel(short, 0.2), lambda: kf.score_poses(Dev(), short),
                 lambda: kf.relocalize_global(Dev(), short)):
        with pytest.raises(AssertionError):
            call()
    cases = [
        (lambda: kf.render_views(np.zeros((2, 3, 4), f32)), "xs_kf_render_views: c2vs must be [P, 4, 4] or [P, 4, 4, 2]"),
        (lambda: kf.render_map(kf.other, np.zeros((0, 4, 4), f32)), "xs_kf_render_map: c2vs must be [P, 4, 4] or [P, 4, 4, 2]"),
        (lambda: kf.render_checkpoint(PATH, POSES, outputs=("depth", "colour")), "xs_kf_render_checkpoint: outputs must name some of depth, depth_u16, normal, shade, counts"),
        (lambda: kf.render_views(POSES, outputs=()), "xs_kf_render_views: outputs must name some of depth, depth_u16, normal, shade, counts"),
        (lambda: kf.sample(POINTS, outputs=("status", "depth")), "xs_kf_sample_points: outputs must name some of status, value, dvalue, gradient, counts"),
        (lambda: kf.sample_map(kf.other, POINTS[:, :2]), "xs_kf_sample_map: points must be [N, 3]"),
        (lambda: kf.sample_checkpoint(PATH, np.zeros((0, 3), f32)), "xs_kf_sample_checkpoint: at least one point is needed"),
        (lambda: kf.register_points(POINTS.reshape(-1)), "xs_kf_register_points: points must be [N, 3]"),
        (lambda: kf.score_map_point_transforms(kf.other, np.zeros((0, 3)), TS), "xs_kf_score_point_transforms_map: at least one point is needed"),
        (lambda: kf.register_checkpoint_points_global(PATH, POINTS[:, :2]), "xs_kf_register_points_global_checkpoint: points must be [N, 3]"),
        (lambda: kf.fuse_points(POINTS[:, :1]), "xs_kf_fuse_points: points must be [N, 3]"),
        (lambda: kf.fuse_points(POINTS, origin=(0.0, 1.0)), "xs_kf_fuse_points: origin must have three entries"),
        (lambda: kf.frame_residuals(np.zeros((2, 3), u16), np.zeros((3, 4))), "frame_residuals: c2v must be [4, 4] or [4, 4, 2]"),
        (lambda: kf.frame_residuals(np.zeros(6, u16), POSES[0]), "frame_residuals: depth must be [rows, cols]"),
        (lambda: kf.frame_residuals(np.zeros((2, 3), u16), POSES[0], outputs=("shade",)), "xs_kf_frame_residuals: outputs must name some of status, value, dvalue, gradient, counts"),
        (lambda: kf.reintegrate_batch([], POSES[:0], POSES[:0]), "reintegrate: at least one frame, one mode per frame"),
        (lambda: kf.reintegrate_batch([1, 2], POSES[:1], POSES), "reintegrate: one camera2volume [4, 4, 2] per frame"),
        (lambda: kf.reintegrate_batch([1, 2], POSES, POSES, frames=[3]), "reintegrate: one frame index (or None) per frame"),
    ]
    for call, text in cases:
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == text
    assert fakes.calls == []


def test_capacity_retry_runs_once_more_with_the_count_reported(kf, fakes):
    fakes.install("xs_kf_path_to", d_path, [-4, 5])
    points, voxels = kf.path_to(POSES[0], 0.2, capacity=8)
    assert [r["capacity"] for _, r in fakes.calls] == [8, 37] and points.shape == (5, 3) and voxels.shape == (5, 3) and voxels[4, 2] == 15
    del fakes.calls[:]
    fakes.install("xs_kf_frontiers", d_frontiers, [-4, 1])
    out = kf.frontiers()
    assert [r["capacity"] for _, r in fakes.calls] == [1024, 37] and out.shape == (5,) and np.array_equal(out["label"], fakes.calls[1][1]["rec"][:, 0])
    del fakes.calls[:]
    fakes.install("xs_kf_propose_views", d_propose, [-4, 1])
    c2vs, cluster = kf.propose_views(0.2)
    assert [r["capacity"] for _, r in fakes.calls] == [1024, 37] and c2vs.shape == (5, 4, 4, 2) and cluster.shape == (5,)
    del fakes.calls[:]
    for s in (1, 2):
        install_family(fakes, "diff", [-4, 1])
        out = call_family(kf, "diff", s)
        assert fakes.names() == [FAMILIES["diff"][0][s]] * 2 and [r["capacity"] for _, r in fakes.calls] == [16, 37]
        assert out.only_this.shape == (5,) and out.only_other.shape == (3,) and np.array_equal(out.only_other["label"], fakes.calls[1][1]["rec1"][:, 0])
        del fakes.calls[:]
    # a second -4 is not run a third time: it is the call's own error
    fakes.install("xs_kf_frontiers", d_frontiers, [-4])
    with pytest.raises(ValueError) as e:
        kf.frontiers()
    assert str(e.value) == "xs_kf_frontiers: -4" and len(fakes.calls) == 2


def test_the_binding_table_is_bound_on_the_shared_library():
    for name, (restype, argtypes) in pl._SIGS.items():
        f = getattr(pl._lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
