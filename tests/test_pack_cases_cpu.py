"""CPU-only: the model the brick-sparse checkpoint is held to (tests/pack_cases.py) against the consequences of the contract (pack then unpack
is the identity, whole and by brick ranges cut inside runs; the writer's files read back), the host's validation of XSTSDF3 through
xs_host_checkpoint_info against the model's reader on good and bad files, x-slam_amd/host/pack_host.hpp under the sanitizers, the bindings, and
the compression the format exists for on the CPU oracle's map."""
import importlib
import os
import subprocess

import numpy as np
import pytest

import pack_cases as pc
from helpers import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pl():
    return importlib.import_module("x-slam_amd.pipeline")


def test_cases_are_what_the_module_says():
    """Every brick has the class it was built for, all eight classes occur in every case of eight bricks and more, and the special contents are there:
    -0.0 beside +0.0, two NaN payloads, one NaN pattern throughout a uniform array, negative weights."""
    seen = set()
    for shape in pc.SHAPES:
        (v, w, g), want = pc.volume(shape)
        cls, offsets, payload = pc.expected(shape)
        assert np.array_equal(cls, want), shape
        assert int(offsets[-1]) == len(payload) == int(pc.class_words(cls).sum())
        if len(cls) >= 8:
            assert set(cls.tolist()) == set(range(8)), shape
        seen |= set(cls.tolist())
    assert seen == set(range(8))
    (v, w, g), _ = pc.volume((72, 16, 8))
    cls = pc.expected((72, 16, 8))[0]
    assert (v == pc.NEG_ZERO).any() or (g == pc.NEG_ZERO).any() or (w == pc.NEG_ZERO).any()
    assert any((a == pc.NAN_B).any() for a in (v, w, g))
    assert (w.view(np.int32) < 0).any()
    nan_uniform = [b for b in range(len(cls)) if not cls[b] & 1 and v[0, 8 * (b // 9):8 * (b // 9) + 1, 8 * (b % 9)][0] == pc.NAN_A]
    assert nan_uniform, "no brick whose value array is one NaN pattern throughout"


def test_one_word_decides():
    """A brick that is uniform but for local voxel (1, 0, 0), or (7, 7, 7), or the last in-volume voxel of a ragged brick, is dense; +0.0 beside
    -0.0 and two NaN payloads are dense; one NaN pattern throughout is uniform; words outside the volume are never compared."""
    for shape, spot in (((8, 8, 8), (0, 0, 1)), ((8, 8, 8), (7, 7, 7)), ((13, 11, 10), (9, 10, 12)), ((13, 11, 10), (1, 2, 4))):
        z = np.full(shape[::-1], 7, np.uint32)
        for a in range(3):
            arrs = [z.copy(), z.copy(), z.copy()]
            assert not pc.classify(*arrs)[0].any()
            arrs[a][spot] ^= 1 << 31
            cls = pc.classify(*arrs)[0]
            b = (spot[0] // 8 * pc.grid(shape)[1] + spot[1] // 8) * pc.grid(shape)[0] + spot[2] // 8
            want = np.zeros_like(cls)
            want[b] = 1 << a
            assert np.array_equal(cls, want), (shape, spot, a)
    f = np.zeros((8, 8, 8), np.float32)
    f[3, 3, 3] = -0.0
    assert pc.classify(f, f, f)[0][0] == 7 and (f == 0).all()
    n = np.full((8, 8, 8), pc.NAN_A, np.uint32)
    assert pc.classify(n, n, n)[0][0] == 0
    m = n.copy()
    m[0, 0, 1] = pc.NAN_B
    assert pc.classify(m, n, m)[0][0] == 5


@pytest.mark.parametrize("shape", pc.SHAPES)
def test_pack_then_unpack_is_the_identity(shape):
    """Whole, and by brick ranges cut inside runs: the ranges' payloads concatenate to the whole payload, and unpacking them one by one into
    sentinel-filled arrays gives the source back word for word."""
    (v, w, g), _ = pc.volume(shape)
    cls, offsets, payload = pc.expected(shape)
    for ranges in pc.splits(len(cls)):
        parts = [pc.gather(v, w, g, cls, offsets, b0, b1) for b0, b1 in ranges]
        assert np.array_equal(np.concatenate(parts), payload)
        out = tuple(np.full(v.shape, 0xA5A5A5A5, np.uint32) for _ in range(3))
        for (b0, b1), part in zip(ranges, parts):
            pc.unpack(out, cls, offsets, part, b0, b1)
        assert all(np.array_equal(o, s) for o, s in zip(out, (v, w, g)))
    # positions of a dense array outside the volume hold the first voxel's word: the payload is a function of the volume's bits alone
    assert np.array_equal(pc.gather(v.copy(), w.copy(), g.copy(), cls, offsets), payload)


@pytest.mark.parametrize("shape", pc.SHAPES)
def test_writer_then_reader_round_trips(shape, pl):
    """The file's length is the formula's, the reader returns the volume, and xs_host_checkpoint_info (the host's validation, no GPU) accepts the file
    and reports what the model's reader reports."""
    (v, w, g), _ = pc.volume(shape)
    cls, offsets, payload = pc.expected(shape)
    poses = bytes(range(128)) * 2
    blob = pc.write_xstsdf3(v, w, g, voxel_size=0.02, tranc_dist=0.06, frame_id=5, poses=poses)
    assert len(blob) == 88 + 256 + -(-len(cls) // 4) * 4 + 4 * len(payload)
    r = pc.read_xstsdf3(blob)
    assert all(np.array_equal(a, b) for a, b in zip(r["volume"], (v, w, g))) and r["poses"] == poses and np.array_equal(r["cls"], cls)
    assert np.array_equal(r["offsets"], offsets)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "a.ckpt")
        open(p, "wb").write(blob)
        info = pl.checkpoint_info(p)
    assert info["version"] == 3 and info["valid"] and info["error"] == "ok"
    assert info["res"] == shape and info["planes"] == (0, shape[2]) and info["shard"] == (0, 1) and info["frame_id"] == 5 and info["n_poses"] == 2
    assert info["voxel_size"] == float(np.float32(0.02)) and info["tranc_dist"] == float(np.float32(0.06))
    assert info["brick_edge"] == 8 and info["brick_grid"] == pc.grid(shape) and info["bricks"] == len(cls)
    assert info["classes"] == np.bincount(cls, minlength=8).tolist() and info["payload_words"] == len(payload) and info["file_bytes"] == len(blob)


def test_a_shard_ranks_planes(pl, tmp_path):
    """Planes [24, 41) of a 17 x 9 x 64 volume: the brick grid is anchored at the first stored plane."""
    (v, w, g), _ = pc.volume((17, 9, 17))
    blob = pc.write_xstsdf3(v, w, g, res=(17, 9, 64), zs0=24, shard=(1, 3))
    r = pc.read_xstsdf3(blob)
    assert r["planes"] == (24, 41) and r["brick_grid"] == (3, 2, 3) and all(np.array_equal(a, b) for a, b in zip(r["volume"], (v, w, g)))
    p = str(tmp_path / "rank1.ckpt")
    open(p, "wb").write(blob)
    info = pl.checkpoint_info(p)
    assert info["valid"] and info["planes"] == (24, 41) and info["shard"] == (1, 3) and info["brick_grid"] == (3, 2, 3) and info["res"] == (17, 9, 64)


def test_bad_files_are_rejected(pl, tmp_path):
    """Each file breaks one rule: the model's reader and xs_host_checkpoint_info both refuse it, and name the same rule.  A dense XSTSDF2 file of
    the same geometry is accepted as version 2; its truncation is not."""
    (v, w, g), _ = pc.volume((17, 9, 10))
    blob = pc.write_xstsdf3(v, w, g)
    bad, dense = pc.bad_files(blob)
    assert set(bad) >= {"truncated", "trailing", "class_8", "payload_words", "reserved", "brick_edge", "grid", "v2_body"}
    rule = {"truncated": "length", "trailing": "length", "class_8": "class_byte", "payload_words": "payload_words", "reserved": "reserved",
            "brick_edge": "brick_edge", "grid": "brick_grid", "nbricks": "brick_grid"}
    for name, data in bad.items():
        with pytest.raises(ValueError) as e:
            pc.read_xstsdf3(data)
        p = str(tmp_path / (name + ".ckpt"))
        open(p, "wb").write(data)
        info = pl.checkpoint_info(p)
        assert info["version"] == 3 and not info["valid"], name
        if name in rule:
            assert info["error"] == rule[name] == str(e.value), (name, info["error"], str(e.value))
    p = str(tmp_path / "dense.ckpt")
    open(p, "wb").write(dense)
    info = pl.checkpoint_info(p)
    assert info["version"] == 2 and info["valid"] and info["res"] == (17, 9, 10) and info["payload_words"] == 3 * 17 * 9 * 10 and "classes" not in info
    open(p, "wb").write(dense[:-4])
    assert not pl.checkpoint_info(p)["valid"]
    for junk in (b"", b"XSTSDF3", b"XSTSDF1\0" + blob[8:]):
        open(p, "wb").write(junk)
        with pytest.raises(ValueError):
            pl.checkpoint_info(p)
    with pytest.raises(ValueError):
        pl.checkpoint_info(str(tmp_path / "missing.ckpt"))


def test_partition_covers_every_brick():
    """The model's partition (what pack_host.hpp's pack_chunk_end is held to in the self-test): no gap, no chunk above the staging words, and
    no chunk that one more brick would still fit into."""
    cls, offsets, _ = pc.expected((72, 16, 8))
    for staging in (1536, 1537, 2000, 4096, 10 ** 6):
        ch = pc.chunk_ends(offsets, staging)
        assert ch[0][0] == 0 and ch[-1][1] == len(cls) and all(a[1] == b[0] for a, b in zip(ch[:-1], ch[1:]))
        for b0, b1 in ch:
            assert b1 > b0 and int(offsets[b1]) - int(offsets[b0]) <= staging
            assert b1 == len(cls) or int(offsets[b1 + 1]) - int(offsets[b0]) > staging


def test_host_code_runs_clean_under_sanitizers(tmp_path):
    """x-slam_amd/host/pack_host.hpp compiled with -fsanitize=address,undefined -fno-sanitize-recover and run (tests/cxx/pack_selftest.cpp)."""
    exe = str(tmp_path / "pack_selftest")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-Wall", "-Werror",
           "-I" + os.path.join(ROOT, "x-slam_amd", "host"), os.path.join(ROOT, "tests", "cxx", "pack_selftest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "all checks held" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_sizes_and_bindings(pl):
    """The brick count and the workspace (a header and one 64-bit sum per 4096 bricks), 0 for what the calls refuse; the entry points of every layer."""
    capi = importlib.import_module("x-slam_amd.capi")
    sh = importlib.import_module("x-slam_amd.sharded")
    for s in pc.SHAPES + [pc.BIG, (512, 512, 512), (1024, 1024, 1024)]:
        assert capi.tsdf_pack_bricks(s) == pc.nbricks(s), s
        n = capi.tsdf_pack_workspace_bytes(s)
        assert n % 256 == 0 and 256 + 8 * -(-pc.nbricks(s) // 4096) <= n <= 512 + 8 * -(-pc.nbricks(s) // 4096), (s, n)
    assert capi.tsdf_pack_bricks((17, 9, 64), planes=17) == 3 * 2 * 3
    for bad in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (4, 300000, 4), (300000, 4, 4), (8, 65536, 32768)):
        assert capi.tsdf_pack_bricks(bad) == 0 and capi.tsdf_pack_workspace_bytes(bad) == 0, bad
    assert capi.tsdf_pack_bricks((8, 8, 8), planes=0) == 0 and capi.tsdf_pack_bricks((8, 8, 8), planes=300000) == 0
    for n in ("xs_tsdf_pack_bricks", "xs_tsdf_pack_workspace_bytes", "xs_tsdf_pack_classify", "xs_tsdf_pack_offsets", "xs_tsdf_pack_gather", "xs_tsdf_unpack"):
        assert n in capi._SIGS and hasattr(capi._lib, n), n
    for n in ("xs_kf_save_checkpoint_sparse", "xs_kf_checkpoint_staging_words", "xs_host_checkpoint_info"):
        assert n in pl._SIGS and hasattr(pl._lib, n), n
    assert capi.abi_version() == 3
    for cls in (pl.KinectFusion, sh.ShardedKinectFusion):
        assert callable(cls.save_checkpoint) and callable(cls.load_checkpoint)
    assert callable(pl.checkpoint_info) and callable(capi.tsdf_unpack)
    assert "either format" in pl.KinectFusion.merge_checkpoint.__doc__ and "either format" in pl.KinectFusion.diff_checkpoint.__doc__


def test_the_oracles_map_compresses(oracle):
    """The condition the format exists for, on the CPU oracle's map: 64^3, six frames of S1.  The model's payload is below a quarter of the dense
    12 bytes per voxel (measured when the format was proposed: 0.085), and bricks of class 0 and of class 7 both occur."""
    from oracle.oracle import OracleKinFu, params_from_dict
    n = 64
    prm = synth.s1_params(n)
    ok = OracleKinFu(oracle, params_from_dict(prm))
    for k in range(6):
        assert ok.process_frame(synth.s1_frame(k)) == 1
    v, w, g = (np.ascontiguousarray(a).reshape(n, n, n) for a in ok.volume())
    assert v.dtype == np.float32 and w.dtype == np.int32 and g.dtype == np.float32
    cls, offsets = pc.classify(v, w, g)
    ratio = 4 * int(offsets[-1]) / (12 * n ** 3)
    hist = np.bincount(cls, minlength=8)
    print(f"payload / dense = {ratio:.4f}; bricks per class {hist.tolist()}")
    assert ratio < 0.25
    assert hist[0] >= 1 and hist[7] >= 1
    out = tuple(np.full((n, n, n), 0xA5A5A5A5, np.uint32) for _ in range(3))
    pc.unpack(out, cls, offsets, pc.gather(v, w, g, cls, offsets))
    assert all(np.array_equal(o, pc.words(s)) for o, s in zip(out, (v, w, g)))
