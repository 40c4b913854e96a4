"""The cases that hold a kernel implementation (the CPU oracle on the CPU suite, the HIP kernels through the C ABI on
the GPU suite) against tests/independent_f64.py: values against the float64 model, CSFD derivatives (imaginary parts / h)
against float64 central differences.  Test infrastructure."""
import ctypes as C

import numpy as np

import independent_f64 as ind
from helpers import intr_of, s1_transforms, synth, tranc_dist

H, W = synth.HEIGHT, synth.WIDTH
Hs = 1e-7          # first-order seed step (Internal.h:33-34)
FD = 1e-5          # central-difference step of the float64 model (metres / radians of the seeded pose entry)


class OracleBackend:
    """oracle/ (complex<float> CPU restatement) behind the interface the cases use."""
    def __init__(self, oracle):
        self.o = oracle

    def scale_depth(self, d):
        return self.o.scale_depth(d)

    def integrate(self, state, depth_m, prm, T, threshold):
        n = prm["tsdf_size_x"]
        v, w, g = (a.copy() for a in state)
        self.o.integrate(depth_m, v, w, g, [n, n, n], tranc_dist(prm), 100, T["Rv2c"], T["tv2c"], intr_of(prm), prm["tsdf_voxel_size"],
                         threshold=threshold)
        return v, w, g

    def raycast(self, state, prm, T):
        n = prm["tsdf_size_x"]
        vm, nm, hits = self.o.raycast(intr_of(prm), T["Rc2v"], T["tc2v"], T["Rv2w"], T["tv2w"], tranc_dist(prm), [n, n, n],
                                      prm["tsdf_voxel_size"], state[0], state[2], H, W)
        return vm, nm, hits

    def current_maps(self, depth_u16, prm, level):
        d = self.o.bilateral(depth_u16)
        for _ in range(level):
            d = self.o.pyr_down(d)
        v = self.o.create_vmap(intr_of(prm, level), d)
        return v, self.o.create_nmap(v)

    def resize(self, vm, nm):
        return self.o.resize_map(vm, False), self.o.resize_map(nm, True)

    def m3_inverse(self, R):
        return self.o.m3_inverse(R)

    def icp(self, Rcurr, tcurr, cv, cn, Rprev_inv, tprev, k, pv, pn, dist, angle):
        s, _, _, inl = self.o.icp_combined(Rcurr, tcurr, cv, cn, Rprev_inv, tprev, k, pv, pn, dist, angle)
        return s, inl

    def hessian(self, depth_m, prm, R36, t12, gt, z0=0, z1=None, res=None, misalign=False):
        res = _res(prm, res)
        return self.o.tsdf_hessian(depth_m, res, prm["tsdf_voxel_size"], R36, t12, tranc_dist(prm), intr_of(prm), gt, z0=z0, z1=z1)

    def gn_terms(self, depth_m, prm, Rs, ts, gt, z0=0, z1=None, res=None, misalign=False):
        res = _res(prm, res)
        return self.o.tsdf_gn_terms(depth_m, res, prm["tsdf_voxel_size"], Rs, ts, tranc_dist(prm), intr_of(prm), gt, z0=z0, z1=z1)


    # ---- map preparation on pitched host buffers (tests/map_cases.py: Pitched), explicit rows / cols and byte pitches ----
    def _a(self, buf, u16=False):
        return C.cast(buf.addr, C.POINTER(C.c_uint16 if u16 else C.c_float))

    def bilateral_p(self, src, dst, rows, cols):
        self.o._bilateral(self._a(src, True), src.pitch, rows, cols, self._a(dst), dst.pitch)

    def pyr_down_p(self, src, dst, srows, scols):
        self.o._pyr_down(self._a(src), src.pitch, srows, scols, self._a(dst), dst.pitch)

    def create_vmap_p(self, intr, depth, vmap, rows, cols):
        k = np.ascontiguousarray(intr, np.float32)
        self.o._create_vmap(k.ctypes.data_as(C.POINTER(C.c_float)), self._a(depth), depth.pitch, rows, cols, self._a(vmap), vmap.pitch)

    def create_nmap_p(self, vmap, nmap, rows, cols):
        assert vmap.pitch == nmap.pitch                                 # one map_step in the ABI
        self.o._create_nmap(rows, cols, self._a(vmap), self._a(nmap), vmap.pitch)

    def resize_p(self, src, dst, srows, scols, normalize):
        self.o._resize_map(1 if normalize else 0, srows, scols, self._a(src), src.pitch, self._a(dst), dst.pitch)

    def create_vnmaps_p(self, intrs, depths, vmaps, nmaps, rows0, cols0, vreal=None, nreal=None):
        """The oracle has no fused launch: per level createVMap then createNMap (what the launch stands for), the real planes copied
        from what those wrote."""
        for l, (k, d, v, n) in enumerate(zip(intrs, depths, vmaps, nmaps)):
            rows, cols = rows0 >> l, cols0 >> l
            self.create_vmap_p(k, d, v, rows, cols)
            self.create_nmap_p(v, n, rows, cols)
            for cplx, real in ((v, vreal), (n, nreal)):
                if real is not None:
                    c, r = cplx.image[..., 0], real[l].image
                    keep = np.tile(np.isnan(c[:rows]), (3, 1))
                    keep[:rows] = False
                    r[...] = np.where(keep, r, c)

    def resize_pyramid_p(self, vmap0, nmap0, rows0, cols0, vmap1, nmap1, vmap2, nmap2):
        for m0, m1, m2, nrm in ((vmap0, vmap1, vmap2, False), (nmap0, nmap1, nmap2, True)):
            self.resize_p(m0, m1, rows0, cols0, nrm)
            self.resize_p(m1, m2, rows0 // 2, cols0 // 2, nrm)

    # ---- ICP reduction on pitched host buffers (tests/icp_cases.py) ----
    def icp_p(self, Rcurr, tcurr, cv, cn, Rprev_inv, tprev, intr, pv, pn, rows, cols, dist, angle, y0=0, y1=None, real=None):
        """The 54 sums and the inlier count of pixel rows [y0, y1): four maps of one pitch.  The oracle reads no float planes: real =
        (vertex, normal) planes stand for complex maps with zero imaginary parts and are expanded into such, at the maps' pitch."""
        from map_cases import Pitched
        assert cv.pitch == cn.pitch == pv.pitch == pn.pitch
        if real is not None:
            cplx = []
            for r in real:
                b = Pitched(3 * rows, cols, np.float32, 2, cv.pitch)
                b.image[..., 0], b.image[..., 1] = r.image, 0.0
                cplx.append(b)
            cv, cn = cplx
        f = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in (Rcurr, tcurr, Rprev_inv, tprev, intr)]
        P = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
        out = np.zeros(55, np.float64)
        out[54] = self.o._icp_combined(P(f[0]), P(f[1]), self._a(cv), self._a(cn), P(f[2]), P(f[3]), P(f[4]), self._a(pv), self._a(pn), cv.pitch,
                                       rows, cols, dist, angle, y0, rows if y1 is None else y1, out.ctypes.data_as(C.POINTER(C.c_double)), None, None)
        return out


class GpuBackend:
    """The HIP kernels through the C ABI (x-slam_amd/capi.py)."""
    def __init__(self, torch, capi, host_m3_inverse):
        self.t, self.c, self._inv = torch, capi, host_m3_inverse

    def dev(self, a):
        a = np.ascontiguousarray(a)
        return self.t.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()

    def scale_depth(self, d):
        out = self.t.zeros((H, W), dtype=self.t.float32, device="cuda")
        self.c.scale_depth(self.dev(d), W * 2, H, W, out, W * 4)
        self.t.cuda.synchronize()
        return out.cpu().numpy()

    def integrate(self, state, depth_m, prm, T, threshold):
        n = prm["tsdf_size_x"]
        v, w, g = (self.dev(a) for a in state)
        self.c.integrate_scaled(self.dev(depth_m), W * 4, H, W, intr_of(prm), 100, [n, n, n], prm["tsdf_voxel_size"], T["Rv2c"], T["tv2c"],
                                tranc_dist(prm), v, w, g, n * 4, threshold=threshold)
        self.t.cuda.synchronize()
        return v.cpu().numpy(), w.cpu().numpy(), g.cpu().numpy()

    def raycast(self, state, prm, T):
        n = prm["tsdf_size_x"]
        vm = self.t.zeros((3 * H, W, 2), dtype=self.t.float32, device="cuda")
        nm = self.t.zeros_like(vm)
        hits = self.t.zeros(1, dtype=self.t.int64, device="cuda")
        self.c.raycast(intr_of(prm), T["Rc2v"], T["tc2v"], T["Rv2w"], T["tv2w"], tranc_dist(prm), [n, n, n], prm["tsdf_voxel_size"],
                       self.dev(state[0]), self.dev(state[2]), n * 4, vm, nm, W * 8, H, W, hits=hits)
        self.t.cuda.synchronize()
        return vm.cpu().numpy(), nm.cpu().numpy(), int(hits.item())

    def current_maps(self, depth_u16, prm, level):
        t, c = self.t, self.c
        rows, cols = H, W
        d = t.zeros((rows, cols, 2), dtype=t.float32, device="cuda")
        c.bilateral_filter(self.dev(depth_u16), W * 2, H, W, d, W * 8)
        for _ in range(level):
            nd = t.zeros((rows // 2, cols // 2, 2), dtype=t.float32, device="cuda")
            c.pyr_down(d, cols * 8, rows, cols, nd, (cols // 2) * 8)
            d, rows, cols = nd, rows // 2, cols // 2
        v = t.zeros((3 * rows, cols, 2), dtype=t.float32, device="cuda")
        nm = t.zeros_like(v)
        c.create_vmap(intr_of(prm, level), d, cols * 8, rows, cols, v, cols * 8)
        c.create_nmap(v, nm, cols * 8, rows, cols)
        t.cuda.synchronize()
        return v.cpu().numpy(), nm.cpu().numpy()

    def resize(self, vm, nm):
        t, c = self.t, self.c
        rows, cols = vm.shape[0] // 3, vm.shape[1]
        ov = t.zeros((3 * (rows // 2), cols // 2, 2), dtype=t.float32, device="cuda")
        on = t.zeros_like(ov)
        c.resize_vmap(self.dev(vm), cols * 8, rows, cols, ov, (cols // 2) * 8)
        c.resize_nmap(self.dev(nm), cols * 8, rows, cols, on, (cols // 2) * 8)
        t.cuda.synchronize()
        return ov.cpu().numpy(), on.cpu().numpy()

    def m3_inverse(self, R):
        return self._inv(R)

    def icp(self, Rcurr, tcurr, cv, cn, Rprev_inv, tprev, k, pv, pn, dist, angle):
        t, c = self.t, self.c
        rows, cols = cv.shape[0] // 3, cv.shape[1]
        ws = t.zeros(c.icp_workspace_bytes(), dtype=t.uint8, device="cuda")
        sums = t.zeros(55, dtype=t.float64, device="cuda")
        c.icp_accumulate(Rcurr, tcurr, self.dev(cv), self.dev(cn), Rprev_inv, tprev, k, self.dev(pv), self.dev(pn), cols * 8, rows, cols, dist, angle,
                         ws, sums)
        t.cuda.synchronize()
        s = sums.cpu().numpy()
        return s[:54], int(s[54])

    def map(self, gt, misalign):
        """gt on the device: at a 16-byte aligned address, or (misalign) at one that is only 4-byte aligned (the one-column scan)."""
        if not misalign:
            return self.dev(gt)
        gt = np.ascontiguousarray(gt, np.float32)
        store = self.t.zeros(gt.size + 5, dtype=self.t.float32, device="cuda")
        out = store[5:5 + gt.size]
        out.copy_(self.t.from_numpy(gt))
        assert out.data_ptr() % 16 == 4
        return out

    def hessian(self, depth_m, prm, R36, t12, gt, z0=0, z1=None, res=None, misalign=False):
        t, c = self.t, self.c
        res = _res(prm, res)
        z1 = res[2] if z1 is None else z1
        ws = t.zeros(c.tsdf_reduce_workspace_bytes(), dtype=t.uint8, device="cuda")
        out = t.zeros(4, dtype=t.float64, device="cuda")
        c.compute_local_tsdf_hessian(self.dev(depth_m), W * 4, H, W, intr_of(prm), res, prm["tsdf_voxel_size"], R36, t12, tranc_dist(prm),
                                     self.map(gt, misalign), ws, out, z0=z0, z1=z1)
        t.cuda.synchronize()
        return out.cpu().numpy()

    def gn_terms(self, depth_m, prm, Rs, ts, gt, z0=0, z1=None, res=None, misalign=False):
        t, c = self.t, self.c
        res = _res(prm, res)
        z1 = res[2] if z1 is None else z1
        ws = t.zeros(c.tsdf_reduce_workspace_bytes(), dtype=t.uint8, device="cuda")
        out = t.full((32,), -1.0, dtype=t.float64, device="cuda")
        c.tsdf_gauss_newton_terms(self.dev(depth_m), W * 4, H, W, intr_of(prm), res, prm["tsdf_voxel_size"], Rs, ts, tranc_dist(prm),
                                  self.map(gt, misalign), ws, out, z0=z0, z1=z1)
        t.cuda.synchronize()
        return out.cpu().numpy()[:29]

    def gn_terms_band(self, depths_m, prm, RsF, tsF, gt, res=None):
        """The band pass (xs_tsdf_gauss_newton_terms_band) for F = len(depths_m) frames over the index of the whole map gt: [F, 29]."""
        t, c = self.t, self.c
        res = _res(prm, res)
        F = len(depths_m)
        idx = c.tsdf_band_build(self.dev(gt), res)
        ws = t.zeros(c.tsdf_band_workspace_bytes(F), dtype=t.uint8, device="cuda")
        out = t.full((29 * F,), -1.0, dtype=t.float64, device="cuda")
        ds = [self.dev(d) for d in depths_m]
        c.tsdf_gauss_newton_terms_band(ds, W * 4, H, W, intr_of(prm), prm["tsdf_voxel_size"], np.stack(RsF), np.stack(tsF), tranc_dist(prm), idx, ws, out)
        t.cuda.synchronize()
        return out.cpu().numpy().reshape(F, 29)


    # ---- map preparation on pitched buffers (tests/map_cases.py: Pitched): the whole buffer, guard rows and padding included, goes
    # to the device and comes back; the kernels get the address of image row 0 ----
    def _up(self, *bufs):
        ts = [self.t.from_numpy(b.a).cuda() for b in bufs]
        return ts, [t.data_ptr() + b.pitch for t, b in zip(ts, bufs)]

    def _down(self, bufs, ts):
        self.t.cuda.synchronize()
        for b, t in zip(bufs, ts):
            b.a[...] = t.cpu().numpy()

    def bilateral_p(self, src, dst, rows, cols):
        ts, (s, d) = self._up(src, dst)
        self.c.bilateral_filter(s, src.pitch, rows, cols, d, dst.pitch)
        self._down([dst], ts[1:])

    def pyr_down_p(self, src, dst, srows, scols):
        ts, (s, d) = self._up(src, dst)
        self.c.pyr_down(s, src.pitch, srows, scols, d, dst.pitch)
        self._down([dst], ts[1:])

    def create_vmap_p(self, intr, depth, vmap, rows, cols):
        ts, (s, d) = self._up(depth, vmap)
        self.c.create_vmap(intr, s, depth.pitch, rows, cols, d, vmap.pitch)
        self._down([vmap], ts[1:])

    def create_nmap_p(self, vmap, nmap, rows, cols):
        assert vmap.pitch == nmap.pitch
        ts, (s, d) = self._up(vmap, nmap)
        self.c.create_nmap(s, d, vmap.pitch, rows, cols)
        self._down([nmap], ts[1:])

    def resize_p(self, src, dst, srows, scols, normalize):
        ts, (s, d) = self._up(src, dst)
        (self.c.resize_nmap if normalize else self.c.resize_vmap)(s, src.pitch, srows, scols, d, dst.pitch)
        self._down([dst], ts[1:])

    def create_vnmaps_p(self, intrs, depths, vmaps, nmaps, rows0, cols0, vreal=None, nreal=None):
        bufs = list(depths) + list(vmaps) + list(nmaps) + (list(vreal) + list(nreal) if vreal is not None else [])
        ts, ps = self._up(*bufs)
        n = len(depths)
        kw = {}
        if vreal is not None:
            kw = dict(vreal=ps[3 * n:4 * n], nreal=ps[4 * n:5 * n], real_steps=[b.pitch for b in vreal])
            assert [b.pitch for b in vreal] == [b.pitch for b in nreal]
        assert [b.pitch for b in vmaps] == [b.pitch for b in nmaps]
        self.c.create_vnmaps(intrs, ps[:n], [b.pitch for b in depths], rows0, cols0, ps[n:2 * n], ps[2 * n:3 * n], [b.pitch for b in vmaps], **kw)
        self._down(bufs[n:], ts[n:])

    def resize_pyramid_p(self, vmap0, nmap0, rows0, cols0, vmap1, nmap1, vmap2, nmap2):
        bufs = [vmap0, nmap0, vmap1, nmap1, vmap2, nmap2]
        assert vmap0.pitch == nmap0.pitch and vmap1.pitch == nmap1.pitch and vmap2.pitch == nmap2.pitch
        ts, ps = self._up(*bufs)
        self.c.resize_pyramid(ps[0], ps[1], vmap0.pitch, rows0, cols0, ps[2], ps[3], vmap1.pitch, ps[4], ps[5], vmap2.pitch)
        self._down(bufs[2:], ts[2:])

    # ---- ICP reduction on pitched buffers (tests/icp_cases.py) ----
    def _pinned(self, nbytes):
        """nbytes of zeroed host-coherent pinned memory: (address, free)."""
        hip = C.CDLL("libamdhip64.so")
        p = C.c_void_p()
        assert hip.hipHostMalloc(C.byref(p), C.c_size_t(nbytes), C.c_uint(0x40000000 | 0x2)) == 0
        C.memset(p, 0, nbytes)
        return p.value, lambda: hip.hipHostFree(p)

    def icp_p(self, Rcurr, tcurr, cv, cn, Rprev_inv, tprev, intr, pv, pn, rows, cols, dist, angle, y0=0, y1=None, real=None, form="device",
              posted=False, launches=1):
        """The 55 doubles of one launch over pixel rows [y0, y1).  real = (vertex, normal) float planes: the _real entry points, which are
        then given no complex current maps.  form: 'device' (sums in device memory), 'pairs' (XS_ICP_PUBLISH_PAIRS into pinned memory) or
        'records' (xs_icp_accumulate_records + xs_icp_sum_records; the records are left in self.records).  posted: the pose comes through
        a mailbox, posted before anything synchronises.  launches > 1: the same launch again on the same workspace, which must give the
        same bits.  Every input buffer must come back byte-identical, guard rows and padding included."""
        t, c = self.t, self.c
        y1 = rows if y1 is None else y1
        bufs = [cv, cn, pv, pn] + (list(real) if real is not None else [])
        assert cv.pitch == cn.pitch == pv.pitch == pn.pitch and (real is None or real[0].pitch == real[1].pitch)
        ts, ps = self._up(*bufs)
        tail = (Rprev_inv, tprev, intr, ps[2], ps[3], cv.pitch, rows, cols, dist, angle)
        ws = t.zeros(c.icp_workspace_bytes(), dtype=t.uint8, device="cuda")
        frees, outs = [], []
        try:
            mailbox = None
            if posted:
                mailbox, in_dev = c.icp_mailbox_alloc()
                frees.append(lambda: c.icp_mailbox_free(mailbox, in_dev))
            for k in range(launches):
                seq = 11 + k
                if form == "records":
                    assert not posted and real is None
                    rec, free = self._pinned(c.icp_records_bytes())
                    frees.append(free)
                    c.icp_accumulate_records(Rcurr, tcurr, ps[0], ps[1], *tail, rec, seq, y0=y0, y1=y1)
                    t.cuda.synchronize()
                    count = c.icp_records_count(cols, y0, y1)
                    rc, got = c.icp_sum_records(rec, count, seq, max_spins=1000)      # (the launch has completed: nothing to wait for)
                    assert rc == 0
                    self.records = np.ctypeslib.as_array((C.c_double * (count * 56)).from_address(rec)).reshape(count, 56).copy()
                    outs.append(got)
                    continue
                if form == "pairs":
                    sums, free = self._pinned(1024)
                    frees.append(free)
                    kw = dict(done_flag=c.ICP_PUBLISH_PAIRS, done_seq=seq)
                else:
                    sums, kw = t.full((55,), 7.0, dtype=t.float64, device="cuda"), {}
                if posted and real is not None:
                    c.icp_accumulate_posted_real(mailbox, seq, ps[4], ps[5], real[0].pitch, *tail, ws, sums, y0=y0, y1=y1, **kw)
                elif posted:
                    c.icp_accumulate_posted(mailbox, seq, ps[0], ps[1], *tail, ws, sums, y0=y0, y1=y1, **kw)
                elif real is not None:
                    assert form == "device"
                    c.icp_accumulate_real(Rcurr, tcurr, ps[4], ps[5], real[0].pitch, *tail, ws, sums, y0=y0, y1=y1)
                else:
                    c.icp_accumulate(Rcurr, tcurr, ps[0], ps[1], *tail, ws, sums, y0=y0, y1=y1, **kw)
                if posted:
                    c.icp_post_pose(mailbox, Rcurr, tcurr, seq)                     # before anything waits for the launch
                t.cuda.synchronize()
                if form == "pairs":
                    rc, got = c.icp_wait_pairs(sums, seq, max_spins=1000)
                    assert rc == 0
                    outs.append(got)
                else:
                    outs.append(sums.cpu().numpy())
        finally:
            t.cuda.synchronize()
            for free in frees:
                free()
        for o in outs[1:]:
            assert np.array_equal(o.view(np.uint64), outs[0].view(np.uint64)), "a repeated launch must give the same bits"
        for b, d in zip(bufs, ts):
            assert np.array_equal(d.cpu().numpy(), b.a), "the launch wrote to an input buffer"
        return outs[0]


def _res(prm, res):
    n = prm["tsdf_size_x"]
    return [n, n, n] if res is None else [int(r) for r in res]


def _frame(scene, k):
    return synth.s3_frame(k) if scene == "s3" else synth.s1_frame(k)


def _flat_to_zyx(a, n):
    return np.asarray(a).reshape(n, n, n)


def two_frames(be, n, scene, seed, threshold):
    """Volume after frames 0 and 1 (each with the seeded pose of its frame), through the implementation under test."""
    prm = synth.s1_params(n, seed=seed, threshold=threshold)
    state0 = (np.zeros(n ** 3, np.float32), np.zeros(n ** 3, np.int32), np.zeros(n ** 3, np.float32))
    out = [state0]
    for k in (0, 1):
        T = s1_transforms(k, prm, seed=seed)
        out.append(be.integrate(out[-1], be.scale_depth(_frame(scene, k)), prm, T, threshold))
    return prm, out


def check_integrate(be, n=128, scene="s3", seed=(2, 3), threshold=0.0, samples=200000, rng_seed=1):
    """Voxel update of frame 1 on top of frame 0: every sampled voxel the kernel wrote, value and d/dseed."""
    prm, states = two_frames(be, n, scene, seed, threshold)
    T = s1_transforms(1, prm, seed=seed)
    depth_m = be.scale_depth(_frame(scene, 1))
    (v0, w0, g0), (v1, w1, g1) = states[1], states[2]
    rng = np.random.default_rng(rng_seed)
    written = np.nonzero(w1 != w0)[0]
    band = written[np.abs(v1[written]) < 0.999]                       # inside the truncation band: the voxels that carry a derivative
    pick = np.unique(np.concatenate([rng.choice(written, min(samples, written.size), replace=False),
                                     rng.choice(band, min(samples, band.size), replace=False),
                                     rng.choice(n ** 3, samples // 4, replace=False)]))
    xyz = np.stack([pick % n, (pick // n) % n, pick // (n * n)], -1)
    args = (T["Rv2c"], T["tv2c"], xyz, depth_m, intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm), threshold, v0[pick], g0[pick], w0[pick])
    f0, dec = ind.integrate(0.0, Hs, *args)
    fp, _ = ind.integrate(+FD, Hs, *args, dec=dec)
    fm, _ = ind.integrate(-FD, Hs, *args, dec=dec)
    dmodel = (fp - fm) / (2 * FD)
    upd_impl = w1[pick] != w0[pick]
    upd_model = dec["update"]
    m = upd_impl & upd_model
    got_v, got_d = v1[pick][m].astype(np.float64), g1[pick][m].astype(np.float64) / Hs
    scale_d = np.abs(dmodel[m]).max()
    out = dict(n_voxels=int(m.sum()), n_band=int((np.abs(f0[m]) < 0.999).sum()),
               written_disagree=float((upd_impl != upd_model).mean()),
               value_bad=float((np.abs(got_v - f0[m]) > 2e-5).mean()), value_err_p999=float(np.quantile(np.abs(got_v - f0[m]), 0.999)),
               deriv_scale=float(scale_d),
               deriv_bad=float((np.abs(got_d - dmodel[m]) > 1e-3 * scale_d).mean()),
               deriv_err_p999_rel=float(np.quantile(np.abs(got_d - dmodel[m]), 0.999) / scale_d),
               bilinear_share=float(dec["bil"][m].mean()))
    return out


def check_raycast(be, n=128, scene="s3", seed=(2, 3), threshold=0.0, samples=20000, rng_seed=2):
    """Rays of the pose of frame 2 into the volume of frames 0-1: vertex and normal maps, values and d/dseed."""
    prm, states = two_frames(be, n, scene, seed, threshold)
    state = states[2]
    T = s1_transforms(2, prm, seed=seed)
    vm, nm, hits = be.raycast(state, prm, T)
    rng = np.random.default_rng(rng_seed)
    pix = np.sort(rng.choice(H * W, samples, replace=False))
    py, px = pix // W, pix % W
    vol, grd = _flat_to_zyx(state[0], n), _flat_to_zyx(state[2], n)
    args = (intr_of(prm), T["Rc2v"], T["tc2v"], T["Rv2w"], T["tv2w"], tranc_dist(prm), [n, n, n], prm["tsdf_voxel_size"], vol, grd, px, py)
    v0, n0, dec = ind.raycast(0.0, Hs, *args)
    vp, np_, _ = ind.raycast(+FD, Hs, *args, dec=dec)
    vm_, nm_, _ = ind.raycast(-FD, Hs, *args, dec=dec)
    dv, dn = (vp - vm_) / (2 * FD), (np_ - nm_) / (2 * FD)
    gv = np.stack([vm[py + p * H, px] for p in range(3)], 1)          # [samples, 3, 2]
    gn = np.stack([nm[py + p * H, px] for p in range(3)], 1)
    hit_impl, nrm_impl = ~np.isnan(gv[:, 0, 0]), ~np.isnan(gn[:, 0, 0])
    both = hit_impl & dec["hit"]
    bn = nrm_impl & dec["has_normal"] & both
    ev = np.abs(gv[both][:, :, 0] - v0[both]).max(-1)
    en = np.abs(gn[bn][:, :, 0] - n0[bn]).max(-1)
    sdv, sdn = np.abs(dv[both]).max(), np.abs(dn[bn]).max()
    edv = np.abs(gv[both][:, :, 1] / Hs - dv[both]).max(-1)
    edn = np.abs(gn[bn][:, :, 1] / Hs - dn[bn]).max(-1)
    return dict(hits=int(hits), n_hit=int(both.sum()), hit_disagree=float((hit_impl != dec["hit"]).mean()),
                normal_disagree=float((nrm_impl[both] != dec["has_normal"][both]).mean()),
                vertex_bad=float((ev > 2e-5).mean()), vertex_err_p99=float(np.quantile(ev, 0.99)),
                normal_bad=float((en > 2e-3).mean()), normal_err_p99=float(np.quantile(en, 0.99)),
                dvertex_scale=float(sdv), dvertex_bad=float((edv > 2e-2 * sdv).mean()), dvertex_err_p99_rel=float(np.quantile(edv, 0.99) / sdv),
                dnormal_scale=float(sdn), dnormal_bad=float((edn > 5e-2 * sdn).mean()), dnormal_err_p99_rel=float(np.quantile(edn, 0.99) / sdn))


def check_icp(be, n=128, scene="s3", seed=(2, 3), threshold=0.0, level=0):
    """27 complex sums of one ICP iteration (frame 2 against the model maps raycast at the pose of frame 1).  The current-frame maps and
    the resized model maps are the backend's own; they are themselves held against the float64 model in tests/map_cases.py."""
    prm, states = two_frames(be, n, scene, seed, threshold)
    T1 = s1_transforms(1, prm, seed=seed)
    pv, pn, _ = be.raycast(states[2], prm, T1)
    for _ in range(level):
        pv, pn = be.resize(pv, pn)
    cv, cn = be.current_maps(_frame(scene, 2), prm, level)
    k = intr_of(prm, level)
    Rprev_inv = be.m3_inverse(T1["Rc2w"])
    angle = float(np.sin(np.float32(15.0) / np.float32(180.0) * np.pi))
    sums, inl = be.icp(T1["Rc2w"], T1["tc2w"], cv, cn, Rprev_inv, T1["tc2w"], k, pv, pn, 0.10, angle)
    args = (T1["Rc2w"], T1["tc2w"], cv, cn, Rprev_inv, T1["tc2w"], k, pv, pn, 0.10, angle)
    s0, inl0, dec = ind.icp_normal_equations(0.0, Hs, *args)
    sp, _, _ = ind.icp_normal_equations(+FD, Hs, *args, dec=dec)
    sm, _, _ = ind.icp_normal_equations(-FD, Hs, *args, dec=dec)
    ds = (sp - sm) / (2 * FD)
    re, im = sums[0::2], sums[1::2] / Hs
    return dict(inliers=int(inl), inliers_model=int(inl0), value_err_rel=float(np.abs(re - s0).max() / np.abs(s0).max()),
                deriv_scale=float(np.abs(ds).max()), deriv_err_rel=float(np.abs(im - ds).max() / np.abs(ds).max()))


def dual_pose(prm, k, h=1e-6):
    """volume-to-camera pose of frame k as dual-complex groups with both first-order seeds on t_x (tests/golden/make_golden.py: hessian)."""
    w2v = np.eye(4)
    w2v[:3, 3] = [prm["init_x"], prm["init_y"], prm["init_z"]]
    v2c = np.linalg.inv(w2v @ synth.s1_pose(k))
    R = np.zeros((3, 3, 4), np.float32)
    R[..., 0] = v2c[:3, :3]
    t = np.zeros((3, 4), np.float32)
    t[:, 0] = v2c[:3, 3]
    t[0, 1] = h
    t[0, 2] = h
    return R, t


def check_hessian(be, n=128, scene="s3", k=1, z0=0, z1=None, gt=None, fd=2e-4):
    """Dual-complex local-TSDF residual: loss, d/dt_x and d2/dt_x^2 of the sum of squared errors against the TSDF of frame 0."""
    prm = synth.s1_params(n)
    h2 = 1e-6                                                           # DoubleComplex.cpp:61-66
    if gt is None:
        _, states = two_frames(be, n, scene, (0, 3), 0.0)
        gt = states[1][0]
    depth_m = be.scale_depth(_frame(scene, k))
    R, t = dual_pose(prm, k, h2)
    out = be.hessian(depth_m, prm, R, t, gt if z1 is None else gt[z0 * n * n:z1 * n * n], z0, z1)
    g3 = _flat_to_zyx(gt, n)[z0:z1]
    args = (R, t, g3, depth_m, intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm), z0)
    l0, c0, dec = ind.tsdf_residual_loss(0.0, h2, *args)
    lp, _, _ = ind.tsdf_residual_loss(+fd, h2, *args, dec=dec)
    lm, _, _ = ind.tsdf_residual_loss(-fd, h2, *args, dec=dec)
    g_model, h_model = (lp - lm) / (2 * fd), (lp - 2 * l0 + lm) / (fd * fd)
    return dict(count=float(out[3]), count_model=c0, loss=float(out[0]), loss_model=l0, grad=float(out[1] / h2), grad_model=g_model,
                hess=float(out[2] / h2 / h2), hess_model=h_model)


# ------------------------------------------------------------------------------------------------
# Pose seeds along se(3) generators, the residual kernels' second-order and six-pose forms
HSTEP = np.float32(1e-7)   # first-order seed of the six Gauss-Newton poses (the orchestrator's)
H2 = 1e-6                  # dual-complex seed of the Hessian kernel (DoubleComplex.cpp:61-66)
# Central-difference step of the seeded-pose models.  With the decisions held, a bilinear depth lookup whose four taps straddle a depth
# edge is strongly curved in the pose (its a * b term): on scene S1 at 64^3, 2e-4 leaves truncation errors of 1e-2 of sqrt(|H_aa H_bb|)
# on rotation pairs and 2e-2 on a rotation gradient; from 2e-6 down the model sits on the kernels' float32 floor, and float64 round-off
# stays far below it.
FD2 = 1e-6


def generator(k):
    """se(3) generator k of the twist (t_x, t_y, t_z, omega_x, omega_y, omega_z) as a 4 x 4 matrix."""
    G = np.zeros((4, 4))
    if k < 3:
        G[k, 3] = 1
    else:
        w = np.zeros(3); w[k - 3] = 1
        G[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return G


def seeded_v2c(v2c):
    """The six complex v2c poses v2c exp(-i h G_k), first order in h: [6, 3, 3, 2], [6, 3, 2] float32."""
    Rs = np.zeros((6, 3, 3, 2), np.float32); ts = np.zeros((6, 3, 2), np.float32)
    for k in range(6):
        d = -v2c @ generator(k)          # d/deps inverse(exp(eps G) c2v) at 0
        Rs[k, :, :, 0] = v2c[:3, :3]; Rs[k, :, :, 1] = HSTEP * d[:3, :3]
        ts[k, :, 0] = v2c[:3, 3]; ts[k, :, 1] = HSTEP * d[:3, 3]
    return Rs, ts


def seeded_poses(c2v_real):
    """The six complex v2c poses the orchestrator builds: inverse(se3Exp(i h e_k) c2v), first order in h."""
    return seeded_v2c(np.linalg.inv(c2v_real))


def frame_v2c(prm, k, rng=None, scale=1.0):
    """Volume-to-camera pose of frame k as float64 holding float32 values (dual_pose's real part), optionally moved by a random twist."""
    R, t = dual_pose(prm, k)
    v2c = np.eye(4)
    v2c[:3, :3], v2c[:3, 3] = R[..., 0], t[:, 0]
    if rng is not None:
        xi = rng.normal(size=6) * scale * np.array([0.01, 0.01, 0.01, 0.004, 0.004, 0.004])
        v2c = (v2c @ _expm(-_hat(xi))).astype(np.float32).astype(np.float64)
    return v2c


def _hat(xi):
    return sum(x * generator(k) for k, x in enumerate(xi))


def _expm(A, terms=20):
    out, term = np.eye(4), np.eye(4)
    for i in range(1, terms):
        term = term @ A / i
        out = out + term
    return out


def pair_pose(v2c, a, b, h=H2, cross=False):
    """Dual-complex pose (Rv2c [3, 3, 4], tv2c [3, 4] float32) of L(v2c exp(-theta_a G_a - theta_b G_b)): real part v2c, eps1 = h (-v2c G_a),
    eps2 = h (-v2c G_b) and, with cross, eps1 eps2 = h^2 v2c (G_a G_b + G_b G_a) / 2 — then hessian / h^2 is the exact entry d2L / dtheta_a
    dtheta_b; without it, the Gauss-Newton-style entry of the linearised pose."""
    Ga, Gb = generator(a), generator(b)
    parts = [v2c, -h * v2c @ Ga, -h * v2c @ Gb, (h * h * v2c @ (Ga @ Gb + Gb @ Ga) / 2) if cross else np.zeros((4, 4))]
    R = np.stack([m[:3, :3] for m in parts], -1).astype(np.float32)
    t = np.stack([m[:3, 3] for m in parts], -1).astype(np.float32)
    return R, t


def pair_model(R, t, args, h=H2, fd=FD2, dec=None):
    """The float64 model of one Hessian launch: loss and count at the real pose, d/dp1, the four-point mixed stencil
    (f(+,+) - f(+,-) - f(-,+) + f(-,-)) / 4 fd^2 and the two diagonals (the tolerance scale) of f(p1, p2) = the loss at
    seeded_pose((p1, p2)).  dec: the decisions of an earlier call at the same real pose (they do not depend on the seeds)."""
    l0, c0, dec = ind.tsdf_residual_loss((0.0, 0.0), h, R, t, *args, dec=dec)
    f = lambda p1, p2: ind.tsdf_residual_loss((p1, p2), h, R, t, *args, dec=dec)[0]
    fa = f(fd, 0.0), f(-fd, 0.0)
    fb = f(0.0, fd), f(0.0, -fd)
    return dict(loss=l0, count=c0, grad=(fa[0] - fa[1]) / (2 * fd),
                h_ab=(f(fd, fd) - f(fd, -fd) - f(-fd, fd) + f(-fd, -fd)) / (4 * fd * fd),
                h_aa=(fa[0] - 2 * l0 + fa[1]) / (fd * fd), h_bb=(fb[0] - 2 * l0 + fb[1]) / (fd * fd)), dec


def pair_errors(out, m, h=H2):
    """A Hessian launch's out4 against pair_model, each on its tolerance scale: loss relative, gradient on max(|g|, sqrt(loss |H_aa|)),
    H_ab on sqrt(|H_aa H_bb|)."""
    grad, hess = float(out[1]) / h, float(out[2]) / h / h
    return dict(count=float(out[3]), count_model=m["count"], loss=float(out[0]), loss_model=m["loss"], grad=grad, grad_model=m["grad"],
                hess=hess, hess_model=m["h_ab"], h_aa=m["h_aa"], h_bb=m["h_bb"],
                loss_err_rel=abs(float(out[0]) - m["loss"]) / abs(m["loss"]),
                grad_err=abs(grad - m["grad"]) / max(abs(m["grad"]), (m["loss"] * abs(m["h_aa"])) ** 0.5),
                hess_err=abs(hess - m["h_ab"]) / abs(m["h_aa"] * m["h_bb"]) ** 0.5)


def crop(gt, n, res):
    """The corner [0, X) x [0, Y) x [0, Z) of a cubic n^3 map (flat), flat: the same voxels at the same coordinates in a smaller map."""
    X, Y, Z = res
    return np.ascontiguousarray(_flat_to_zyx(gt, n)[:Z, :Y, :X]).reshape(-1)


def residual_inputs(be, n=64, scene="s3", k=1, gt=None):
    """Map of frames 0-1 (through the implementation under test), scaled depth of frame k."""
    if gt is None:
        _, states = two_frames(be, n, scene, (0, 3), 0.0)
        gt = states[1][0]
    return synth.s1_params(n), gt, be.scale_depth(_frame(scene, k))


def perturbed_v2c(prm, k, perturb):
    """frame_v2c of frame k, moved by a fixed random twist of perturb times (1 cm, 0.004 rad) per component when perturb > 0.  Near the
    map's optimum the loss's gradient is small, and with it the part the eps1 eps2 input adds to H_ab (1e-4 .. 4e-4 of sqrt(|H_aa H_bb|) on
    S1 at the frame's own pose); three units away it is 1e-3 and more."""
    return frame_v2c(prm, k, np.random.default_rng(5), perturb) if perturb else frame_v2c(prm, k)


def check_hessian_pair(be, a, b, n=64, scene="s3", k=1, cross=False, perturb=0.0, z0=0, z1=None, gt=None, res=None, misalign=False, fd=FD2):
    """One Hessian launch with eps1 along se(3) generator a and eps2 along b (pair_pose) at perturbed_v2c against pair_model.  gt: the whole
    map (flat, X * Y * Z of res, default the n^3 map of frames 0-1); [z0, z1) the planes the launch takes."""
    prm, gt, depth_m = residual_inputs(be, n, scene, k, gt)
    X, Y, Z = _res(prm, res)
    z1 = Z if z1 is None else z1
    R, t = pair_pose(perturbed_v2c(prm, k, perturb), a, b, cross=cross)
    slab = gt[z0 * X * Y:z1 * X * Y]
    out = be.hessian(depth_m, prm, R, t, slab, z0, z1, res=[X, Y, Z], misalign=misalign)
    args = (slab.reshape(z1 - z0, Y, X), depth_m, intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm), z0)
    m, _ = pair_model(R, t, args, fd=fd)
    return pair_errors(out, m)


def check_full_hessian(be, n=128, scene="s3", k=1, cross=(), perturb=0.0, fd=FD2):
    """The 6 x 6 Hessian at perturbed_v2c from 21 launches (pairs a <= b; the pairs in cross also with the eps1 eps2 input), each against
    its model; the decisions are taken once for all (one real pose).  Returns the per-entry figures and the worst of each."""
    prm, gt, depth_m = residual_inputs(be, n, scene, k)
    v2c = perturbed_v2c(prm, k, perturb)
    args = (_flat_to_zyx(gt, n), depth_m, intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm), 0)
    dec, entries = None, {}
    for a in range(6):
        for b in range(a, 6):
            for c in (False, True) if (a, b) in cross else (False,):
                R, t = pair_pose(v2c, a, b, cross=c)
                out = be.hessian(depth_m, prm, R, t, gt)
                m, dec = pair_model(R, t, args, fd=fd, dec=dec)
                entries[f"{a}{b}{'x' if c else ''}"] = pair_errors(out, m)
    worst = {key: max(e[key] for e in entries.values()) for key in ("loss_err_rel", "grad_err", "hess_err")}
    counts = [(e["count"], e["count_model"]) for e in entries.values()]
    return dict(entries=entries, worst=worst, count_diff=max(abs(c - cm) for c, cm in counts), count_min=min(c for c, _ in counts),
                count_spread=max(c for c, _ in counts) - min(c for c, _ in counts))


def gn_errors(got, m):
    """29 kernel sums against gn_terms' model, each on its Cauchy-Schwarz scale: J^T J_jk on sqrt(J^T J_jj J^T J_kk), J^T r_k on
    sqrt(J^T J_kk sum r^2), sum r^2 relative."""
    diag = m[[0, 6, 11, 15, 18, 20]]
    jk = [(j, k) for j in range(6) for k in range(j, 6)]
    jtj = max(abs(got[s] - m[s]) / (diag[j] * diag[k]) ** 0.5 for s, (j, k) in enumerate(jk))
    jtr = max(abs(got[21 + k] - m[21 + k]) / (diag[k] * m[27]) ** 0.5 for k in range(6))
    return dict(count=float(got[28]), count_model=float(m[28]), jtj_err=float(jtj), jtr_err=float(jtr),
                r2_err_rel=float(abs(got[27] - m[27]) / m[27]), jtj_diag_min=float(diag.min()))


def check_gn_terms(be, n=64, scene="s3", k=1, z0=0, z1=None, gt=None):
    """The six-pose Gauss-Newton sums (seeded_v2c of frame k's pose) over planes [z0, z1) against gn_terms."""
    prm, gt, depth_m = residual_inputs(be, n, scene, k, gt)
    z1 = n if z1 is None else z1
    Rs, ts = seeded_v2c(frame_v2c(prm, k))
    slab = gt[z0 * n * n:z1 * n * n]
    got = be.gn_terms(depth_m, prm, Rs, ts, slab, z0, z1)
    m = ind.gn_terms(Rs, ts, slab.reshape(z1 - z0, n, n), depth_m, intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm), z0, h=float(HSTEP), fd=FD2)
    return gn_errors(got, m)


def check_gn_band(be, n=128, scene="s3", frames=(1, 2, 3), rng_seed=7):
    """The band pass over the index of the map of frames 0-1, one launch for F = len(frames) frames, each with its own depth frame and
    its own randomly moved pose: every frame's 29 sums against gn_terms for that frame."""
    prm, gt, _ = residual_inputs(be, n, scene, frames[0])
    rng = np.random.default_rng(rng_seed)
    depths, RsF, tsF = [], [], []
    for k in frames:
        depths.append(be.scale_depth(_frame(scene, k)))
        Rs, ts = seeded_v2c(frame_v2c(prm, k, rng))
        RsF.append(Rs); tsF.append(ts)
    got = be.gn_terms_band(depths, prm, RsF, tsF, gt)
    out = []
    for f in range(len(frames)):
        m = ind.gn_terms(RsF[f], tsF[f], _flat_to_zyx(gt, n), depths[f], intr_of(prm), prm["tsdf_voxel_size"], tranc_dist(prm), h=float(HSTEP), fd=FD2)
        out.append(gn_errors(got[f], m))
    return out


def check_hessian_gn_identity(be, n=64, scene="s3", k=1):
    """Two kernels, one derivative: the Hessian launch seeded with eps1 = h (-v2c G_j), eps2 = 0 gives dL/dtheta_j = grad / h, the six-pose
    launch at the same real pose 2 sum d_j r / HSTEP; the difference on the scale 2 sqrt(J^T J_jj sum r^2) / HSTEP, and both counts."""
    prm, gt, depth_m = residual_inputs(be, n, scene, k)
    v2c = frame_v2c(prm, k)
    Rs, ts = seeded_v2c(v2c)
    gn = be.gn_terms(depth_m, prm, Rs, ts, gt)
    diag = gn[[0, 6, 11, 15, 18, 20]]
    errs, counts = [], []
    for j in range(6):
        R, t = pair_pose(v2c, j, j)
        R[..., 2:] = 0; t[:, 2:] = 0
        assert np.array_equal(R[..., 0], Rs[j, ..., 0]) and np.array_equal(t[:, 0], ts[j, :, 0])
        out = be.hessian(depth_m, prm, R, t, gt)
        g_h, g_gn = float(out[1]) / H2, 2.0 * gn[21 + j] / float(HSTEP)
        errs.append(abs(g_h - g_gn) / (2.0 * (diag[j] * gn[27]) ** 0.5 / float(HSTEP)))
        counts.append(float(out[3]))
    return dict(err=float(max(errs)), errs=[float(e) for e in errs], counts=counts, count_gn=float(gn[28]))


# Tolerances of the seeded-pose cases, each on the scale its figure is stated on (pair_errors, gn_errors, check_hessian_gn_identity).
# Measured on the oracle at 64^3 and 128^3 (S3 / S1; the HIP kernels' figures at 128^3 are in profiles/r07_independent_f64.json): H_ab <= 4.4e-5, gradient <= 1.8e-4, loss <= 1.3e-4; J^T J <= 5.2e-5, J^T r <= 9.8e-5,
# sum r^2 <= 6.6e-5; the two kernels' gradients <= 3.1e-5 (both float32 evaluations of one derivative; 1e-4 is that spread with a
# margin of three).
def assert_count(r):
    assert r["count"] > 1000 and abs(r["count"] - r["count_model"]) <= max(2, 1e-4 * r["count_model"]), r


def assert_hessian_pair(r):
    assert_count(r)
    assert r["loss_err_rel"] <= 2e-4, r
    assert r["grad_err"] <= 5e-4, r
    assert r["hess_err"] <= 1e-4, r


def assert_gn(r):
    assert_count(r)
    assert r["jtj_diag_min"] > 0, r
    assert r["jtj_err"] <= 2e-4 and r["jtr_err"] <= 2e-4 and r["r2_err_rel"] <= 2e-4, r


def assert_identity(r):
    assert r["count_gn"] > 1000 and all(c == r["count_gn"] for c in r["counts"]), r
    assert r["err"] <= 1e-4, r
