"""GPU: the kernels of the brick-sparse checkpoint (x-slam_amd/csrc/xs_pack.hip) through capi against the numpy model of tests/pack_cases.py, word for
word: class bytes, offsets and payload on pitched volumes with sentinel-filled padding and guard planes, by brick ranges cut inside runs, the
unpack into sentinel-filled volumes, repeatability, row offsets past 2^31 bytes, and every refusal of the contract."""
import importlib

import numpy as np
import pytest

import merge_cases as mc
import pack_cases as pc

pytestmark = pytest.mark.gpu
SENTINEL = 0x5EA1ED00


@pytest.fixture(scope="module")
def dev():
    import torch
    assert torch.cuda.is_available()
    return torch, importlib.import_module("x-slam_amd.capi")


class Packed:
    """cls, offsets and a payload buffer on the device for one volume, each with sentinel words behind its end."""

    def __init__(self, torch, capi, shape, payload_words):
        self.n = pc.nbricks(shape)
        self.cls = torch.full((self.n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        self.offsets = torch.full((self.n + 1 + 8,), -7, dtype=torch.int64, device="cuda")
        self.payload = torch.full((payload_words + 64,), SENTINEL, dtype=torch.int32, device="cuda")
        self.ws = torch.zeros(capi.tsdf_pack_workspace_bytes(list(shape)), dtype=torch.uint8, device="cuda")

    def host(self, torch):
        torch.cuda.synchronize()
        return self.cls.cpu().numpy(), self.offsets.cpu().numpy().view(np.uint64), self.payload.cpu().numpy().view(np.uint32)


def classify(torch, capi, vol, shape, pk):
    capi.tsdf_pack_classify(vol.value.addr, vol.weight.addr, vol.grad.addr, vol.pitch, list(shape), pk.cls, pk.offsets, pk.ws)


def gather(torch, capi, vol, shape, pk, b0, b1, payload=None):
    capi.tsdf_pack_gather(vol.value.addr, vol.weight.addr, vol.grad.addr, vol.pitch, list(shape), pk.cls, pk.offsets, b0, b1, pk.payload if payload is None else payload)


@pytest.mark.parametrize("shape", pc.SHAPES)
def test_classes_offsets_and_payload_are_the_models(dev, shape):
    """Every pitch of merge_cases.pitches: cls, offsets and the payload word for word, nothing written behind their ends, the volume (guards and
    padding included) untouched; the payload by brick ranges cut inside runs concatenates to the whole; a second run gives equal bytes."""
    torch, capi = dev
    (v, w, g), _ = pc.volume(shape)
    cls, offsets, payload = pc.expected(shape)
    n = len(cls)
    for pitch, offset in mc.pitches(shape[0]):
        vol = mc.DevVolume3(torch, pc.typed((v, w, g)), pitch, offset)
        runs = []
        for _ in range(2):
            pk = Packed(torch, capi, shape, len(payload))
            classify(torch, capi, vol, shape, pk)
            gather(torch, capi, vol, shape, pk, 0, n)
            runs.append(pk.host(torch))
        c, o, p = runs[0]
        assert np.array_equal(c[:n], cls) and (c[n:] == 0xEE).all(), (pitch, offset)
        assert np.array_equal(o[:n + 1], offsets) and (o[n + 1:].view(np.int64) == -7).all()
        assert np.array_equal(p[:len(payload)], payload) and (p[len(payload):] == SENTINEL).all()
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[1]))
        _, ranges = pc.splits(n)
        parts = []
        for b0, b1 in ranges:
            words = int(offsets[b1]) - int(offsets[b0])
            part = torch.full((words + 16,), SENTINEL, dtype=torch.int32, device="cuda")
            gather(torch, capi, vol, shape, pk, b0, b1, part)
            h = part.cpu().numpy().view(np.uint32)
            assert (h[words:] == SENTINEL).all(), (b0, b1)
            parts.append(h[:words])
        assert np.array_equal(np.concatenate(parts), payload)
        assert vol.untouched()


@pytest.mark.parametrize("shape", pc.SHAPES)
def test_offsets_alone_and_unpack(dev, shape):
    """The scan alone on the model's class bytes; the model's payload unpacked into a sentinel-filled volume, whole and range by range: the source
    bit for bit, padding and guard planes as they were; a range writes its own bricks only."""
    torch, capi = dev
    (v, w, g), _ = pc.volume(shape)
    cls, offsets, payload = pc.expected(shape)
    n = len(cls)
    pk = Packed(torch, capi, shape, len(payload))
    pk.cls[:n] = torch.from_numpy(cls.copy()).cuda()
    capi.tsdf_pack_offsets(pk.cls, n, pk.offsets, pk.ws)
    o = pk.host(torch)[1]
    assert np.array_equal(o[:n + 1], offsets) and (o[n + 1:].view(np.int64) == -7).all()
    blank = tuple(np.full(v.shape, 0xA5A5A5A5, np.uint32) for _ in range(3))
    whole, ranges = pc.splits(n)
    for pitch, offset in mc.pitches(shape[0])[1:3]:
        for rs in (whole, ranges):
            out = mc.DevVolume3(torch, pc.typed(blank), pitch, offset)
            so_far = tuple(b.copy() for b in blank)
            for b0, b1 in rs:
                part = torch.from_numpy(payload[int(offsets[b0]):int(offsets[b1])].view(np.int32).copy()).cuda()
                capi.tsdf_unpack(out.value.addr, out.weight.addr, out.grad.addr, out.pitch, list(shape), pk.cls, pk.offsets, b0, b1, part)
                torch.cuda.synchronize()
                pc.unpack(so_far, cls, offsets, payload[int(offsets[b0]):int(offsets[b1])], b0, b1)
                assert out.equals(pc.typed(so_far)), (pitch, rs, b0, b1)
            assert out.equals(pc.typed((v, w, g)))


def test_rows_past_two_gib(dev):
    """pack_cases.BIG at a pitch of 4096 bytes: 2.1 GiB per array, the last planes' rows past 2^31 bytes from the base.  The volume is zero but
    for the first and the last 8 planes, which hold a case volume's bricks: class bytes, offsets and payload are the model's, and the payload
    unpacked into a second, sentinel-filled set of arrays reproduces the first."""
    torch, capi = dev
    X, Y, P = pc.BIG
    pw = pc.BIG_PITCH // 4
    assert (Y * (P - 1) + Y - 1) * pc.BIG_PITCH > 2 ** 31
    (sv, sw, sg), _ = pc.volume((16, 24, 8))
    host = [np.zeros((P, Y, X), np.uint32) for _ in range(3)]
    for h, s in zip(host, (sv, sw, sg)):
        h[:8, :24] = s
        h[P - 8:, Y - 24:] = s
        h[P - 1, Y - 1, X - 1] ^= 1                     # the last voxel of the volume, in a ragged brick (513 = 64 * 8 + 1)
    cls, offsets = pc.classify(*host)
    payload = pc.gather(*host, cls, offsets)
    n = len(cls)
    assert n == 2 * 128 * 65 and cls[-1] == 7 and cls.any() and (cls[300:-2 * 128 * 2] == 0).all()
    src = [torch.full((P * Y, pw), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    dst = [torch.full((P * Y, pw), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(3)]
    for t, h in zip(src, host):
        t[:, :X] = torch.from_numpy(h.view(np.int32).reshape(P * Y, X)).cuda()
    pk = Packed(torch, capi, pc.BIG, len(payload))
    capi.tsdf_pack_classify(src[0], src[1], src[2], pc.BIG_PITCH, list(pc.BIG), pk.cls, pk.offsets, pk.ws)
    capi.tsdf_pack_gather(src[0], src[1], src[2], pc.BIG_PITCH, list(pc.BIG), pk.cls, pk.offsets, 0, n, pk.payload)
    c, o, p = pk.host(torch)
    assert np.array_equal(c[:n], cls) and np.array_equal(o[:n + 1], offsets) and np.array_equal(p[:len(payload)], payload)
    assert (p[len(payload):] == SENTINEL).all()
    half = n // 2 + 3
    for b0, b1 in ((0, half), (half, n)):
        part = pk.payload[int(offsets[b0]):int(offsets[b1])].clone()
        capi.tsdf_unpack(dst[0], dst[1], dst[2], pc.BIG_PITCH, list(pc.BIG), pk.cls, pk.offsets, b0, b1, part)
    torch.cuda.synchronize()
    for s, d in zip(src, dst):
        assert torch.equal(s, d)                        # the volume's words, and the sentinels of the padding


def test_refusals(dev):
    """Every refusal of the contract raises (hipErrorInvalidValue) and writes nothing: outputs and volume keep their bytes."""
    torch, capi = dev
    shape = (17, 9, 10)
    (v, w, g), _ = pc.volume(shape)
    cls, offsets, payload = pc.expected(shape)
    n = len(cls)
    vol = mc.DevVolume3(torch, pc.typed((v, w, g)), 17 * 4 + 4, 0)
    good = Packed(torch, capi, shape, len(payload))
    classify(torch, capi, vol, shape, good)
    gather(torch, capi, vol, shape, good, 0, n)
    before = good.host(torch)
    A = (vol.value.addr, vol.weight.addr, vol.grad.addr)
    P, R = vol.pitch, list(shape)
    fresh = Packed(torch, capi, shape, len(payload))
    blank = fresh.host(torch)
    calls = []
    for k in range(3):                                   # a null array
        a = list(A)
        a[k] = None
        calls.append(lambda a=a: capi.tsdf_pack_classify(a[0], a[1], a[2], P, R, fresh.cls, fresh.offsets, fresh.ws))
        calls.append(lambda a=a: capi.tsdf_pack_gather(a[0], a[1], a[2], P, R, good.cls, good.offsets, 0, n, fresh.payload))
        calls.append(lambda a=a: capi.tsdf_unpack(a[0], a[1], a[2], P, R, good.cls, good.offsets, 0, n, good.payload))
    calls += [lambda: capi.tsdf_pack_classify(*A, P, R, None, fresh.offsets, fresh.ws), lambda: capi.tsdf_pack_classify(*A, P, R, fresh.cls, None, fresh.ws),
              lambda: capi.tsdf_pack_classify(*A, P, R, fresh.cls, fresh.offsets, None),
              lambda: capi.tsdf_pack_offsets(None, n, fresh.offsets, fresh.ws), lambda: capi.tsdf_pack_offsets(good.cls, n, None, fresh.ws),
              lambda: capi.tsdf_pack_offsets(good.cls, n, fresh.offsets, None), lambda: capi.tsdf_pack_offsets(good.cls, 0, fresh.offsets, fresh.ws),
              lambda: capi.tsdf_pack_offsets(good.cls, 1 << 31, fresh.offsets, fresh.ws),
              lambda: capi.tsdf_pack_gather(*A, P, R, None, good.offsets, 0, n, fresh.payload), lambda: capi.tsdf_pack_gather(*A, P, R, good.cls, None, 0, n, fresh.payload),
              lambda: capi.tsdf_pack_gather(*A, P, R, good.cls, good.offsets, 0, n, None),
              lambda: capi.tsdf_unpack(*A, P, R, None, good.offsets, 0, n, good.payload), lambda: capi.tsdf_unpack(*A, P, R, good.cls, None, 0, n, good.payload),
              lambda: capi.tsdf_unpack(*A, P, R, good.cls, good.offsets, 0, n, None)]
    bad_res = [[0, 9, 10], [17, -1, 10], [17, 9, 0], [262141, 9, 10], [17, 262141, 10], [17, 9, 262141]]
    bad_geometry = [(P, r, None) for r in bad_res] + [(P, R, 0), (P, R, -3), (P, R, 262141), (P, [17, 65536, 40000], 32768)]
    bad_geometry += [(17 * 4 - 4, R, None), (17 * 4 + 2, R, None), (0, R, None)]              # a pitch shorter than a row, or no multiple of 4
    for pitch, res, planes in bad_geometry:
        calls.append(lambda a=(pitch, res, planes): capi.tsdf_pack_classify(*A, a[0], a[1], fresh.cls, fresh.offsets, fresh.ws, planes=a[2]))
        calls.append(lambda a=(pitch, res, planes): capi.tsdf_pack_gather(*A, a[0], a[1], good.cls, good.offsets, 0, 1, fresh.payload, planes=a[2]))
        calls.append(lambda a=(pitch, res, planes): capi.tsdf_unpack(*A, a[0], a[1], good.cls, good.offsets, 0, 1, good.payload, planes=a[2]))
    for b0, b1 in ((0, 0), (3, 3), (5, 2), (0, n + 1), (n, n + 1), (n, n)):                  # empty, reversed, outside [0, nbricks]
        calls.append(lambda r=(b0, b1): capi.tsdf_pack_gather(*A, P, R, good.cls, good.offsets, r[0], r[1], fresh.payload))
        calls.append(lambda r=(b0, b1): capi.tsdf_unpack(*A, P, R, good.cls, good.offsets, r[0], r[1], good.payload))
    for i, call in enumerate(calls):
        with pytest.raises(capi.XsError, match="xs_tsdf_(pack|unpack)"):
            call()
    assert len(calls) > 60
    after, untouched = good.host(torch), fresh.host(torch)
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and all(np.array_equal(a, b) for a, b in zip(blank, untouched))
    assert vol.untouched()
