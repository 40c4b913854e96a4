"""bench.py's timed region and --dump-outputs, on the host: the headline's loop driven with a stand-in for the pipeline (no GPU call).
--steps K must time exactly K frames whatever K is (scene S1 stops tracking on one runner after ~530 frames, so a long region runs on
fresh runners), and the dump must hold finite float32 / float64 arrays within its 64 MB."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    return importlib.import_module("bench")


class _Runner:
    """The parts of pipeline.KinectFusion the headline calls; counts the frames processed while the timed region's profiling level is on."""
    made = []

    def __init__(self, prm):
        self.prm, self.res, self.height, self.level, self.timed, self.frames = prm, [32, 32, 32], 480, 0, 0, 0
        _Runner.made.append(self)

    def process_frame(self, depth):
        self.frames += 1
        self.timed += self.level == 1
        return 1

    def hint_next_frame(self, depth):
        pass

    def set_profiling(self, level):
        self.level = level

    def reset_stage_times(self):
        pass

    def cumulative_counters(self):
        return 1000, 0

    def stage_times(self):
        return {s: (0.01, 1) for s in ("surface", "icp", "scale", "integrate", "raycast", "resize")}

    def icp_iteration_times(self):
        return {lv: (1.0, 1) for lv in range(4)}

    def world2camera(self):
        return np.zeros((4, 4, 2), np.float32)

    def volume(self):
        n = 32 ** 3
        return np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)

    def map(self, which, level):
        m = np.ones((3 * 480, 640, 2), np.float32)
        m[:480, :320, 0] = np.nan          # rays without a vertex: the raycast's NaN sentinel, as the pipeline writes it
        return m

    def close(self):
        pass


def _args(steps, warmup, full=True):
    return argparse.Namespace(steps=steps, warmup=warmup, full=full, size=512, scene="s1", replicas=False, force_composite=False, icp_solve=None,
                              no_post_pose=False, icp_lookahead=None, icp_complex_maps=False, no_classify_ahead=False, integrate_post=False,
                              no_integrate_post=False, classify_slack=None, param=[], no_sign_map=False, sign_map_shift=None, icp_fold=None,
                              host_frames=False, no_look_ahead=False, no_legs=True, no_alt=True, icp_shard_rows=False, native_rccl=False)


@pytest.mark.parametrize("steps", [1, 20, 469, 470, 2000])
def test_steps_sets_the_timed_frames(bench, monkeypatch, steps):
    torch = types.SimpleNamespace(from_numpy=lambda a: types.SimpleNamespace(cuda=lambda: a),
                                  cuda=types.SimpleNamespace(synchronize=lambda: None))
    synth = types.SimpleNamespace(s1_frame=lambda k: np.zeros((480, 640), np.uint16), s3_frame=None, s1_params=lambda n: {})
    monkeypatch.setattr(bench, "raycast_figures", lambda *a, **k: {})
    _Runner.made = []
    dump = {}
    out = bench.track(_args(steps, 10), torch, synth, None, types.SimpleNamespace(KinectFusion=_Runner), None, 0, 1, lambda: None, dump)
    headline = [r for r in _Runner.made if r.prm.get("biInterpolate_threshold") != 0.02]
    assert sum(r.timed for r in headline) == steps == out["steps"] == sum(out["segments"]["frames"])
    assert all(r.frames <= 480 + 60 for r in headline)        # no runner is asked to track S1 into its second lap's loss
    assert out["ms_per_step"] > 0 and out["value"] > 0
    assert {"track_world2camera", "track_vmap_model_level0", "track_vmap_model_level0_valid", "track_tsdf_value_sample"} <= set(dump)
    assert all(np.isfinite(v).all() for v in dump.values())
    assert dump["track_vmap_model_level0_valid"].shape == (480, 640) and dump["track_vmap_model_level0_valid"].sum() == 480 * 320
    assert (dump["track_vmap_model_level0"][:480, :320, 0] == 0).all()


@pytest.mark.parametrize("steps", [1, 200, 2000])
def test_plain_run_is_the_timed_steps_alone(bench, monkeypatch, steps):
    """Without --full the headline renders and runs only what its timed steps need: frame 0, the warm-up and the segments on their
    runners (each announcing the frame after its last), none of the per-stage, level-0, raycast or bilinear passes, and no leg."""
    rendered = []

    def frame(k):
        rendered.append(k)
        return np.zeros((480, 640), np.uint16)
    torch = types.SimpleNamespace(from_numpy=lambda a: types.SimpleNamespace(cuda=lambda: a),
                                  cuda=types.SimpleNamespace(synchronize=lambda: None))
    synth = types.SimpleNamespace(s1_frame=frame, s3_frame=None, s1_params=lambda n: {})
    monkeypatch.setattr(bench, "raycast_figures", lambda *a, **k: pytest.fail("raycast figures in a plain run"))
    _Runner.made = []
    out = bench.track(_args(steps, 10, full=False), torch, synth, None, types.SimpleNamespace(KinectFusion=_Runner), None, 0, 1, lambda: None, {})
    segs = out["segments"]["frames"]
    assert sum(segs) == steps == out["steps"] and len(_Runner.made) == len(segs)
    assert [r.frames for r in _Runner.made] == [1 + 10 + k for k in segs] and [r.timed for r in _Runner.made] == segs
    assert rendered == list(range(min(10 + 2 + max(segs), bench.T_PERIOD)))
    assert not {"stages_ms", "raycast", "roofline_icp", "bilinear", "legs", "sustained"} & set(out)
    assert out["ms_per_step"] > 0 and out["value"] > 0 and "roofline" in out and "icp_us_per_iteration" in out


def test_dump_is_float_and_bounded(bench, tmp_path):
    shapes = bench.write_outputs(str(tmp_path), {"a": np.arange(6, dtype=np.int32), "b": np.ones(3, np.float64), "c": np.ones((2, 2), np.float16)})
    assert shapes == {"a": [6], "b": [3], "c": [2, 2]}
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert got["a"].dtype == np.float32 and got["b"].dtype == np.float64 and got["c"].dtype == np.float32
    assert np.array_equal(got["a"], np.arange(6))
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_BYTES // 4 + 1, np.float32)})
    with pytest.raises(AssertionError):
        bench.write_outputs(str(tmp_path / "nan"), {"x": np.array([1.0, np.nan], np.float32)})
