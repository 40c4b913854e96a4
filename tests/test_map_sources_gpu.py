"""GPU: where the calls that take a map get it from, at the C ABI (include/xslam_amd_pipeline.h), at 64^3 on the synthetic scene S3.  Each of
the *_map / *_checkpoint entry points (merge, align, align_global, score_transforms, diff, render, sample, register: sixteen), and the *_volume
and own-map forms of render, sample and register, is called through pipeline._lib with every output filled with a sentinel: with a source the
library refuses (a null or `self` other instance, a null path, a missing file, a file that is not a checkpoint, a null or aliasing array) and
with one valid source.  The return code is asserted, and for a refused call which outputs still hold the sentinel: every one of them, except
the report of the calls that clear it before they look at the source.  Every refused call is one the library refuses cleanly."""
import ctypes as C
import importlib

import numpy as np
import pytest

from helpers import synth

pytestmark = pytest.mark.gpu
N, FRAMES = 64, 3
SENT = 77                    # what every output holds before a call
ROWS, COLS, POINTS = 48, 64, 64


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi"), importlib.import_module("x-slam_amd.pipeline")


@pytest.fixture(scope="module")
def scene(dev, tmp_path_factory):
    """Two instances with the same three frames (a: the source, never modified; k: the caller), a's dense checkpoint, a file that is no
    checkpoint, and points of a's surface."""
    torch, capi, pl = dev
    prm = synth.s1_params(N)
    frames = [torch.from_numpy(synth.s3_frame(i).view(np.int16)).cuda() for i in range(FRAMES)]
    a, k = pl.KinectFusion(prm), pl.KinectFusion(prm)
    for kf in (a, k):
        for f in frames:
            assert kf.process_frame(f) == 1
        kf.synchronize()
    d = tmp_path_factory.mktemp("sources")
    good, junk = str(d / "a.ckpt"), str(d / "junk.ckpt")
    a.save_checkpoint(good)
    with open(junk, "wb") as f:
        f.write(b"not a checkpoint at all " * 64)
    cloud = a.export_point_cloud()[0]
    assert len(cloud) > 4 * POINTS
    pts = np.ascontiguousarray(cloud[:: len(cloud) // POINTS][:POINTS], np.float32)
    yield dict(a=a, k=k, prm=prm, good=good, junk=junk, missing=str(d / "missing.ckpt"), pts=pts, pose=np.ascontiguousarray(a.camera2volume(), np.float32))
    a.close()
    k.close()


def buffers():
    full = lambda shape, dtype: np.full(shape, SENT, dtype)   # noqa: E731
    return dict(written=full(1, np.uint64), T_out=full(16, np.float64), report=full(12, np.float64), hist=full(8, np.float64), out2=full((2, 2), np.float64),
                recs_this=full((16, 8), np.uint64), recs_other=full((16, 8), np.uint64), n_this=full(1, np.int32), n_other=full(1, np.int32),
                counts3=full(3, np.uint64), depth=full((1, ROWS, COLS), np.float32), depth_u16=full((1, ROWS, COLS), np.uint16),
                normal=full((1, 3, ROWS, COLS), np.float32), shade=full((1, ROWS, COLS), np.uint8), rcounts=full((1, 4), np.uint32),
                status=full(POINTS, np.uint8), value=full(POINTS, np.float32), dvalue=full(POINTS, np.float32), gradient=full((POINTS, 3), np.float32),
                scounts=full(4, np.uint64))


def p(arr, ctype=None):
    return arr.ctypes.data if ctype is None else arr.ctypes.data_as(C.POINTER(ctype))


EYE = np.ascontiguousarray(np.eye(4).reshape(1, 16).repeat(2, 0))   # two transforms, both the identity


def merge(pl, s, name, src, b):
    return getattr(pl._lib, name)(s["k"].h, *src, p(EYE, C.c_double), 1, p(b["written"], C.c_ulonglong))


def align(pl, s, name, src, b):
    return getattr(pl._lib, name)(s["k"].h, *src, p(EYE, C.c_double), 1, 2, 1e-3, 1, 1.0, p(b["T_out"], C.c_double), p(b["report"], C.c_double), p(b["hist"], C.c_double))


def align_global(pl, s, name, src, b):
    o = pl.AlignSearchOpts()
    pl._lib.xs_kf_align_search_defaults(s["k"].h, C.byref(o))
    o.candidates, o.keep, o.rounds, o.iterations, o.user_n, o.user_T16xN = 1, 1, 0, 2, 1, p(EYE, C.c_double)   # the caller's one candidate: the identity
    return getattr(pl._lib, name)(s["k"].h, *src, C.byref(o), p(b["T_out"], C.c_double), p(b["report"], C.c_double))


def score_transforms(pl, s, name, src, b):
    return getattr(pl._lib, name)(s["k"].h, *src, 2, p(EYE, C.c_double), 1, 1, 1.0, p(b["out2"], C.c_double))


def diff(pl, s, name, src, b):
    return getattr(pl._lib, name)(s["k"].h, *src, p(EYE, C.c_double), 1, 0.0, 0.5, 0, 8, 16, p(b["recs_this"], C.c_uint64), p(b["n_this"], C.c_int),
                                  p(b["recs_other"], C.c_uint64), p(b["n_other"], C.c_int), p(b["counts3"], C.c_ulonglong), None, None)


def render(pl, s, name, src, b, views=1):
    return getattr(pl._lib, name)(s["k"].h, *src, views, p(s["pose"], C.c_float), 1, None, ROWS, COLS, None, p(b["depth"]), p(b["depth_u16"]), p(b["normal"]),
                                  p(b["shade"]), p(b["rcounts"]), 0)


def sample(pl, s, name, src, b, n=POINTS):
    return getattr(pl._lib, name)(s["k"].h, *src, n, p(s["pts"]), None, 1, p(b["status"]), p(b["value"]), p(b["dvalue"]), p(b["gradient"]), p(b["scounts"]), 0)


def register(pl, s, name, src, b, n=POINTS):
    return getattr(pl._lib, name)(s["k"].h, *src, n, p(s["pts"]), 0, p(EYE, C.c_double), 1, 2, 1e-3, 1, 0.9, p(b["T_out"], C.c_double), p(b["report"], C.c_double),
                                  p(b["hist"], C.c_double))


RENDER_OUT = ("depth", "depth_u16", "normal", "shade", "rcounts")
SAMPLE_OUT = ("status", "value", "dvalue", "gradient", "scounts")
# family: (the call, the outputs a valid call writes, the report words it clears before anything else)
FAMILY = dict(merge=(merge, ("written",), 0), align=(align, ("T_out", "report", "hist"), 8), align_global=(align_global, ("T_out", "report"), 12),
              score_transforms=(score_transforms, ("out2",), 0), diff=(diff, ("n_this", "n_other", "counts3"), 0), render=(render, RENDER_OUT, 0),
              sample=(sample, SAMPLE_OUT, 0), register=(register, ("T_out", "report", "hist"), 7))
# entry point: (family, kind of source, whether the report is cleared BEFORE the source is resolved: a refused source then leaves it cleared)
ENTRY = {
    "xs_kf_merge_map": ("merge", "map", False), "xs_kf_merge_checkpoint": ("merge", "checkpoint", False),
    "xs_kf_align_map": ("align", "map", False), "xs_kf_align_checkpoint": ("align", "checkpoint", True),
    "xs_kf_align_map_global": ("align_global", "map", False), "xs_kf_align_checkpoint_global": ("align_global", "checkpoint", True),
    "xs_kf_score_transforms": ("score_transforms", "map", False), "xs_kf_score_transforms_checkpoint": ("score_transforms", "checkpoint", False),
    "xs_kf_diff_map": ("diff", "map", False), "xs_kf_diff_checkpoint": ("diff", "checkpoint", False),
    "xs_kf_render_map": ("render", "map", False), "xs_kf_render_checkpoint": ("render", "checkpoint", False),
    "xs_kf_sample_map": ("sample", "map", False), "xs_kf_sample_checkpoint": ("sample", "checkpoint", False),
    "xs_kf_register_map": ("register", "map", True), "xs_kf_register_checkpoint": ("register", "checkpoint", True),
}


def cleared(report, words):
    return report[0] == -1.0 and not report[1:words].any() and (report[words:] == SENT).all()


def assert_untouched(b, but_report_words=0, what=""):
    for name, arr in b.items():
        if name == "report" and but_report_words:
            assert cleared(arr, but_report_words), (what, arr)
        else:
            assert (arr == SENT).all(), (what, name)


def assert_written(b, names, what=""):
    for name in names:
        assert not (b[name] == SENT).all(), (what, name)


@pytest.mark.parametrize("name", sorted(n for n, e in ENTRY.items() if e[1] == "map"))
def test_other_instance(dev, scene, name):
    """A null other instance and the caller itself: -1, and only a report that is cleared before the source is looked at has changed.  The
    source instance: 1 (merge goes into an instance of its own)."""
    torch, capi, pl = dev
    family, _, clears_first = ENTRY[name]
    call, outs, words = FAMILY[family]
    for what, other in (("null", None), ("self", scene["k"].h)):
        b = buffers()
        assert call(pl, scene, name, (other,), b) == -1, (name, what)
        assert_untouched(b, words if clears_first else 0, (name, what))
    b = buffers()
    s = scene
    if family == "merge":
        s = dict(scene, k=pl.KinectFusion(scene["prm"]))
    assert call(pl, s, name, (scene["a"].h,), b) == 1, name
    assert_written(b, outs, name)
    if family == "merge":
        assert b["written"][0] > 100
        s["k"].close()
    elif words:
        assert b["report"][0] == 0.0 and (b["report"][words:] == SENT).all()


@pytest.mark.parametrize("name", sorted(n for n, e in ENTRY.items() if e[1] == "checkpoint"))
def test_checkpoint(dev, scene, name):
    """A null path: -1 with every output untouched, the report too.  A missing file and a file that is no checkpoint: -1, and only a report
    that is cleared before the file is opened has changed.  The source's checkpoint: 1."""
    torch, capi, pl = dev
    family, _, clears_first = ENTRY[name]
    call, outs, words = FAMILY[family]
    b = buffers()
    assert call(pl, scene, name, (None,), b) == -1, name
    assert_untouched(b, 0, (name, "null path"))
    for what in ("missing", "junk"):
        b = buffers()
        assert call(pl, scene, name, (scene[what].encode(),), b) == -1, (name, what)
        assert_untouched(b, words if clears_first else 0, (name, what))
    b = buffers()
    s = scene
    if family == "merge":
        s = dict(scene, k=pl.KinectFusion(scene["prm"]))
    assert call(pl, s, name, (scene["good"].encode(),), b) == 1, name
    assert_written(b, outs, name)
    if family == "merge":
        assert b["written"][0] > 100
        s["k"].close()
    elif words:
        assert b["report"][0] == 0.0 and (b["report"][words:] == SENT).all()


def volume_source(kf, grad, value=True):
    """The (value, weight[, grad], step, res, voxel size, truncation distance) arguments of a *_volume call from an instance's own arrays."""
    v, step = kf.volume_ptr("value")
    w, g = kf.volume_ptr("weight")[0], kf.volume_ptr("grad")[0]
    res = (C.c_int * 3)(*kf.res)
    return ((v if value else None, w) + ((g,) if grad else ()) + (step, res, float(np.float32(float(kf.cfg["tsdf_voxel_size"]))), kf.tranc_dist()))


def test_volume_forms(dev, scene):
    """xs_kf_render_volume and xs_kf_sample_volume: a null value array and the caller's own arrays are refused with -1 and nothing written;
    the source's arrays give 1."""
    torch, capi, pl = dev
    a, k = scene["a"], scene["k"]
    for name, call, outs, grad in (("xs_kf_render_volume", render, RENDER_OUT, False), ("xs_kf_sample_volume", sample, SAMPLE_OUT, True)):
        for what, src in (("null value", volume_source(a, grad, value=False)), ("aliasing", volume_source(k, grad))):
            b = buffers()
            assert call(pl, scene, name, src, b) == -1, (name, what)
            assert_untouched(b, 0, (name, what))
        b = buffers()
        assert call(pl, scene, name, volume_source(a, grad), b) == 1, name
        assert_written(b, outs, name)


def test_own_map_forms(dev, scene):
    """xs_kf_render_views, xs_kf_sample_points and xs_kf_register_points on the caller's own map: no view or no point is refused with -1 and
    nothing written (register's report cleared); a view and the points give 1."""
    torch, capi, pl = dev
    for name, call, outs, words in (("xs_kf_render_views", render, RENDER_OUT, 0), ("xs_kf_sample_points", sample, SAMPLE_OUT, 0),
                                    ("xs_kf_register_points", register, ("T_out", "report", "hist"), 7)):
        b = buffers()
        assert call(pl, scene, name, (), b, 0) == -1, name
        assert_untouched(b, words, name)
        b = buffers()
        assert call(pl, scene, name, (), b) == 1, name
        assert_written(b, outs, name)
        if words:
            assert b["report"][0] == 0.0 and (b["report"][words:] == SENT).all()
