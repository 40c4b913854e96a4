/* xslam_amd.h — C ABI of the MI355X-native XKinectFusion CSFD hot path (libxslam_hip.so).
 *
 * Every entry point replaces one launcher function of the reference's kernel-launcher API
 * (XKinectFusion/include/{TsdfVolume.h,TsdfFusion.h,RayCaster.h,ICP.h,Map.h}); the original
 * signature each one stands in for is cited per function.  Plain pointers and sizes only:
 *
 *   - device pointers are raw HIP device addresses; `step` / `*_step` is the row pitch in
 *     BYTES, as in the reference's PtrStep<T> (DeviceArray/include/kernel_containers.hpp:53-55)
 *   - complex values are (re, im) float pairs; MatS33 = 9 pairs row-major (18 floats),
 *     devComplex3 = 3 pairs (6 floats), the layouts device_cast<> reinterprets
 *     (XKinectFusion/include/Internal.h:42-45, 63-65, 146-148); MatD33 / devDComplex3 are
 *     9 / 3 groups of (re.re, re.im, im.re, im.im) (cuda_double_complex.hpp:24-31)
 *   - Intr is float[4] = {fx, fy, cx, cy} (Internal.h:49-59); int3 is int[3] = {x, y, z}
 *   - a vertex/normal map is 3 stacked planes of rows x cols complex (Map.cu:23-25)
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream).  Calls enqueue
 *     work and return; nothing synchronises unless the function says so.  The reference
 *     synchronises the device inside most launchers.
 *   - return value: 0 on success, otherwise the hipError_t code; xs_last_error() gives text.
 *     The reference prints and exit(-1)s on any CUDA error (Common/include/cx.h:125-130);
 *     the C++ shim above this ABI reproduces that.
 */
#ifndef XSLAM_AMD_H
#define XSLAM_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

const char *xs_last_error(void);

/* floor(p / voxel_size) in the raycast march without a divide (a reciprocal product with one fused residual correction), used ONLY
 * for constants that xs_const_div_prepare has checked — on the device, every one of the 2^32 float operands against the divide (~2 ms
 * and one synchronisation per new constant; the verdict is kept in a process-wide table).  Returns bit 1: floor(short form) ==
 * floor(divide) for all |x| <= 2^60 (what the march uses), bit 0: the quotients are bit-identical for 2^-60 <= |x| <= 2^60 and +-0
 * (recorded only); 0: no device / constant outside [2^-20, 2^20].  xs_raycast called with a voxel_size that was never prepared
 * (xs_const_div_state == 0) brackets the quotient with two reciprocal products and divides where they disagree — same results.
 * The orchestrator prepares voxel_size in AllocateBuffers. */
unsigned xs_const_div_prepare(float c);
unsigned xs_const_div_state(float c);
int xs_const_div_enable(int on);   /* test aid: 0 = every launcher divides whatever has been prepared; returns the previous setting */
/* ABI version, bumped on any signature change */
int xs_abi_version(void);

/* ---- TSDF volume ---------------------------------------------------------------------- */
/* initVolume(PtrStep<short2>, PtrStep<float> value, PtrStep<int> weight, PtrStep<float> grad,
 *            const int3&)                                    TsdfVolume.h:16, TsdfFusion.cu:34-43
 * Zero-fills the z-slab [z0, z1) whose storage starts at the given pointers. */
int xs_init_volume(float *value, int *weight, float *grad, size_t step_bytes, const int *res, int z0, int z1, void *stream);

/* scaleDepthKernal launch inside integrateTsdfVolume        TsdfFusion.cu:68-82, :182-187
 * u16 millimetres -> float metres, 0 outside [200, 5000]. */
int xs_scale_depth(const uint16_t *depth, size_t depth_step, int rows, int cols, float *scaled, size_t scaled_step, void *stream);
/* Same, and max_dev (a device float the caller zeroed beforehand) receives the largest valid
 * depth of the frame, for xs_integrate_scaled's far clipping. */
int xs_scale_depth_max(const uint16_t *depth, size_t depth_step, int rows, int cols, float *scaled, size_t scaled_step,
                       float *max_dev, void *stream);
/* Same, and tiles_dev (xs_depth_tiles_bytes(rows, cols) bytes, or NULL) receives the smallest and the largest scaled depth of every
 * 8 x 8 pixel tile {float lo, hi} (an invalid pixel counts as 0).  No counterpart in the reference: the integrate kernel classifies
 * whole bricks from it (free space in front of every surface it can see: written with tsdf = (1, 0) without a projection; behind
 * everything it can see: skipped) and takes the reference's per-voxel path (TsdfFusion.cu:110-167) for the rest — same volume.
 * xs_integrate_opts.depth_tiles hands the table to an xs_integrate_scaled_ex2 / xs_integrate_classify_ex call (NULL: the call builds its
 * own from the scaled image, in its workspace); xs_depth_tiles builds it from an image that is already scaled. */
size_t xs_depth_tiles_bytes(int rows, int cols);
int xs_scale_depth_tiles(const uint16_t *depth, size_t depth_step, int rows, int cols, float *scaled, size_t scaled_step,
                         float *max_dev, void *tiles_dev, void *stream);
int xs_depth_tiles(const float *scaled, size_t scaled_step, int rows, int cols, void *tiles_dev, void *stream);

/* integrateTsdfVolume(const PtrStepSz<ushort>& depth, const Intr&, int max_weight, const int3& res,
 *     float voxel_size, const MatS33& Rv2c, const devComplex3& tv2c, const devComplex3& tc2v,
 *     float tranc_dist, PtrStep<float> value, PtrStep<int> weight, PtrStep<float> grad,
 *     DeviceArray2D<float>& depthScaled, int frame_id, float threshold, float k)
 *                                                            TsdfFusion.h:40-45, TsdfFusion.cu:173-201
 * tc2v, frame_id and k are unused by the reference kernel and are not part of this ABI.
 * depth_scaled: caller-owned rows x cols float workspace.  [z0, z1): the z-slab this device
 * owns (0, res[2] for the whole volume); value/weight/grad point at the slab's storage.
 * updated_dev: optional device counter incremented by the number of voxels written. */
int xs_integrate_tsdf_volume(const uint16_t *depth, size_t depth_step, int rows, int cols, const float *intr4, int max_weight,
                             const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6, float tranc_dist,
                             float *value, int *weight, float *grad, size_t vol_step, float *depth_scaled, size_t scaled_step,
                             float threshold, int z0, int z1, unsigned long long *updated_dev, void *stream);
/* Same, from an already scaled depth image (tsdfFusionKernal alone, TsdfFusion.cu:85-171).
 * depth_max_dev: optional device float = largest valid depth of the frame (xs_scale_depth_max);
 * lets a column stop behind the farthest surface.  NULL = walk the whole frustum. */
int xs_integrate_scaled(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, int max_weight,
                        const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6, float tranc_dist, float *value,
                        int *weight, float *grad, size_t vol_step, float threshold, int z0, int z1,
                        unsigned long long *updated_dev, const float *depth_max_dev, void *workspace, void *stream);
/* xs_integrate_scaled with its two bracketing launches under the caller's control (both are tiny, but each is a dependent
 * dispatch on the stream: ~14 us of a 390 us frame).  flags: XS_INTEGRATE_HEADER_IS_CLEAR — the caller has cleared the
 * workspace header since the previous call (xs_integrate_workspace_clear, on any stream ordered before this call);
 * XS_INTEGRATE_NO_FOLD — the voxel count stays in the workspace (a word per workgroup, behind the header) until the caller folds it into updated_dev
 * (xs_integrate_fold_counts, ordered after this call and before the next clear).  updated_dev non-NULL still enables
 * the counting.  flags = 0 is xs_integrate_scaled. */
#define XS_INTEGRATE_HEADER_IS_CLEAR 1u
#define XS_INTEGRATE_NO_FOLD 2u
#define XS_INTEGRATE_ALWAYS_STORE 8u    /* store all three words of every updated voxel, also where their bits do not change (the default stores only words that change: same volume, fewer bytes) */
/* (16u was the posted launch of ABI 2, whose kernel took its pose from a mailbox: a call that still sets it fails with hipErrorInvalidValue) */
#define XS_INTEGRATE_NO_TILES 32u        /* every brick takes the exact per-voxel walk: no free-space / nothing-to-write classification from the depth tiles (A/B and tests; same volume either way) */
#define XS_INTEGRATE_COUNT_CLASSES 64u   /* the kernel counts the wave-sized boxes it classified: 32-bit words 48 / 49 / 50 of the workspace = free / nothing to write / exact walk (cleared with the header; tests and bench figures) */
#define XS_INTEGRATE_RECLASSIFY_BOXES 128u /* with XS_INTEGRATE_LIST_IS_READY: the brick list holds for this pose but the box classes xs_integrate_classify left do not (xs_integrate_list_covers returned 1, not 3): classify the boxes again, with this pose */
#define XS_INTEGRATE_LIST_IS_READY 4u   /* xs_integrate_classify has produced the brick list on this stream (see there) */
int xs_integrate_scaled_ex(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, int max_weight,
                           const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6, float tranc_dist, float *value,
                           int *weight, float *grad, size_t vol_step, float threshold, int z0, int z1,
                           unsigned long long *updated_dev, const float *depth_max_dev, void *workspace, unsigned flags, void *stream);
int xs_integrate_workspace_clear(void *workspace, void *stream);
int xs_integrate_fold_counts(void *workspace, unsigned long long *updated_dev, void *stream);
/* The brick classification of an integrate call ahead of the call, for a pose that is only NEARLY the final one (the orchestrator
 * enqueues it behind the last ICP launch with the pose that launch starts from: the list is there when the final pose is, and
 * the classification's launch latency leaves the frame's critical path).  The frustum's slack is multiplied by slack_scale (>= 1);
 * xs_integrate_list_covers (host only) says whether such a list holds every brick the final pose would list — if so, call
 * xs_integrate_scaled_ex with XS_INTEGRATE_LIST_IS_READY (| XS_INTEGRATE_HEADER_IS_CLEAR) on the same stream / workspace / slab /
 * image size, else clear the header again (xs_integrate_workspace_clear) and call it without.  flags of xs_integrate_classify:
 * XS_INTEGRATE_HEADER_IS_CLEAR as above.  Results are those of the plain call, bit for bit (the list is a superset; every voxel
 * still takes the exact tests with the final pose).
 * With a depth-tile table named (xs_integrate_opts.depth_tiles) xs_integrate_classify_ex also decides the boxes' classes (free space /
 * nothing to write / per-voxel walk), padded for every pose within the slack's allowances; xs_integrate_list_covers returns 0 (the
 * list does not hold), 1 (the list holds, the classes do not: add XS_INTEGRATE_RECLASSIFY_BOXES to the call's flags) or 3 (both hold).
 * The integrate call takes those classes only when it is an xs_integrate_scaled_ex2 call that names the same table and its own pose lies
 * within their slack (it checks: see the options structs below); otherwise it decides the boxes again with its own pose. */
int xs_integrate_classify(int rows, int cols, const float *intr4, const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6,
                          float tranc_dist, int z0, int z1, const float *depth_max_dev, void *workspace, float slack_scale, unsigned flags,
                          void *stream);
int xs_integrate_list_covers(int rows, int cols, const float *intr4, const int *res, float voxel_size, const float *Rv2c18_list,
                             const float *tv2c6_list, float slack_scale, const float *Rv2c18, const float *tv2c6);
/* Device workspace for xs_integrate_scaled's brick work list, for a slab of nz planes.  With a
 * workspace the kernel first lists the 64x4x8-voxel bricks that can intersect the frustum and
 * then spreads them over all CUs; without one (NULL) each column walks its own clipped range. */
size_t xs_integrate_workspace_bytes(const int *res, int nz);

/* ---- Options structs ---------------------------------------------------------------------------------------------------------------
 * Everything a call takes besides its arguments proper — depth-tile table, sign map, events, pyramid outputs — travels in an
 * options struct that is an argument of the call: xs_integrate_scaled_ex2 / xs_integrate_classify_ex / xs_raycast_ex / xs_raycast_slab_ex /
 * xs_resize_pyramid_ex.  The library keeps NO per-thread state (ABI version 2: the xs_*_set_* functions of version 1 are gone), so nothing
 * a previous call set, or an early return forgot to clear, can leak into a call.  The entry points without a struct (xs_integrate_scaled*,
 * xs_integrate_classify, xs_raycast, xs_raycast_slab, xs_resize_pyramid) are the same calls with an empty one.
 * Zero-initialise a struct, set struct_bytes = sizeof(it), fill what applies.
 *   events      hipEvent_t riding on a kernel's own dispatch (its begin / end: no marker packets on the stream); a stop event alone is a completion
 *               event another stream can wait on.
 *
 * The library remembers, per WORKSPACE, what xs_integrate_classify* last classified into it (pose, slack, slab, volume, camera, band, tile
 * table): a following integrate call with XS_INTEGRATE_LIST_IS_READY on that workspace uses those box classes only if all of that is its
 * own and ITS pose lies within the slack they were padded for, and decides the boxes again with its own pose otherwise —
 * XS_INTEGRATE_RECLASSIFY_BOXES is a hint that saves the check, not a correctness requirement (the brick LIST itself is the caller's claim:
 * xs_integrate_list_covers).  Classifying on one host thread and integrating on another is fine. */
typedef struct xs_integrate_opts {
    unsigned struct_bytes;           /* sizeof(xs_integrate_opts) */
    unsigned flags;                  /* XS_INTEGRATE_* */
    const void *depth_tiles;         /* this frame's xs_scale_depth_tiles table, or NULL (the call builds its own in its workspace) */
    void *signmap;                   /* the sign map the call marks, or NULL */
    void *start_event, *stop_event;  /* hipEvent_t riding on the integrate kernel's dispatch (classify: stop_event = its last dispatch); NULL = none */
} xs_integrate_opts;
int xs_integrate_scaled_ex2(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, int max_weight,
                            const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6, float tranc_dist, float *value,
                            int *weight, float *grad, size_t vol_step, float threshold, int z0, int z1,
                            unsigned long long *updated_dev, const float *depth_max_dev, void *workspace, const xs_integrate_opts *opts, void *stream);
int xs_integrate_classify_ex(int rows, int cols, const float *intr4, const int *res, float voxel_size, const float *Rv2c18, const float *tv2c6,
                             float tranc_dist, int z0, int z1, const float *depth_max_dev, void *workspace, float slack_scale,
                             const xs_integrate_opts *opts, void *stream);
typedef struct xs_raycast_opts {
    unsigned struct_bytes;           /* sizeof(xs_raycast_opts) */
    int signmap_shift;               /* the sign map's brick shift (2..6) */
    const void *signmap;             /* the sign map the march goes by, or NULL (march from t = 0.2) */
    float signmap_tranc_dist;        /* the truncation distance the map was reset for */
    float *pyr_vmap1, *pyr_nmap1;    /* model-map pyramid built by the one-launch form (all four or none) */
    size_t pyr_step1;
    float *pyr_vmap2, *pyr_nmap2;
    size_t pyr_step2;
    void *completion_event;          /* hipEvent_t riding on the one-launch form's dispatch, or NULL */
    int *steps_dev;                  /* measurement: rows x cols ints receiving every ray's march length, or NULL */
    int pyramid_built;               /* OUT: 1 if the call built the pyramid (else launch xs_resize_pyramid) */
} xs_raycast_opts;
int xs_raycast_ex(const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
                  float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step,
                  float *vmap, float *nmap, size_t map_step, int rows, int cols, unsigned long long *hits_dev, float *workspace,
                  xs_raycast_opts *opts, void *stream);
int xs_raycast_slab_ex(const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
                       float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step,
                       int zs0, int zs1, int z0, int z1, float *vmap, float *nmap, size_t map_step, int rows, int cols, int *keys_dev,
                       const xs_raycast_opts *opts, void *stream);
int xs_resize_pyramid_ex(const float *vmap0, const float *nmap0, size_t in_step, int rows0, int cols0, float *vmap1, float *nmap1,
                         size_t mid_step, float *vmap2, float *nmap2, size_t out_step, void *completion_event, void *stream);

/* ---- Dual-complex Hessian / real loss over the volume ----------------------------------- */
size_t xs_tsdf_reduce_workspace_bytes(void);
/* The workspace of the three residual kernels (Hessian, loss, Gauss-Newton terms): its first 256 bytes must be ZERO on first use — call this once after
 * allocating it (or zero-fill it) — and every launch leaves them zero (the last workgroup resets the arrival ticket), so a launch carries no fill of
 * its own.  One launch at a time per workspace; initialise again after a launch that did not complete.  (ABI 2; ABI 1 filled the ticket per launch.) */
int xs_tsdf_reduce_workspace_init(void *workspace, void *stream);
/* float4 ComputeLocalTsdf_hessian(depth, Intr, depthScaled, res, voxel_size, const MatD33& Rv2c,
 *     const devDComplex3& tv2c, tranc_dist, threshold, k, gt, real, grad, hessian, count)
 *                                                  TsdfFusion.h:55-60, TsdfFusion.cu:204-331
 * One fused pass: the reference's kernel + 4 thrust::reduce.  out4_dev = {loss, grad, hessian,
 * count} as doubles.  gt: dense unpitched TSDF of the slab [z0, z1).  The four per-voxel
 * volumes (indexed like gt) are optional: all four or none.  threshold / k are unused by the
 * reference kernel and absent here.  workspace: xs_tsdf_reduce_workspace_bytes(), its first 256 bytes ZERO
 * (xs_tsdf_reduce_workspace_init).  Otherwise no workgroup is elected last and nothing is published: out4_dev
 * keeps its old contents and the call still returns 0.  A host wait on a published result (the orchestrator's,
 * xs_estimate_combined's) reports such a launch as an error instead of spinning. */
int xs_compute_local_tsdf_hessian(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                                  const int *res, float voxel_size, const float *Rv2c36, const float *tv2c12, float tranc_dist,
                                  const float *gt, float *real_out, float *grad_out, float *hess_out, int *count_out, int z0, int z1,
                                  void *workspace, double *out4_dev, void *stream);
/* float2 ComputeLocalTsdf_loss(..., const Mat33& Rv2c, const float3& tv2c, ..., gt, real, count)
 *                                                  TsdfFusion.h:48-52, TsdfFusion.cu:335-447
 * workspace: as xs_compute_local_tsdf_hessian — first 256 bytes ZERO (xs_tsdf_reduce_workspace_init), otherwise
 * nothing is published (out2_dev keeps its old contents, the call still returns 0; a host wait on a published result
 * reports such a launch as an error instead of spinning). */
int xs_compute_local_tsdf_loss(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, const int *res,
                               float voxel_size, const float *Rv2c9, const float *tv2c3, float tranc_dist, const float *gt,
                               float *real_out, int *count_out, int z0, int z1, void *workspace, double *out2_dev, void *stream);

/* ---- Depth / vertex / normal maps (Map.h:16-54) ------------------------------------------ */
/* bilateralFilter(const DeviceArray2D<ushort>& src, MapArr& dst)            Map.cu:155-199, 262-271 */
int xs_bilateral_filter(const uint16_t *src, size_t src_step, int rows, int cols, float *dst, size_t dst_step, void *stream);
/* pyrDown(const MapArr& src, MapArr& dst); dst is (rows/2) x (cols/2)        Map.cu:202-230, 274-283 */
int xs_pyr_down(const float *src, size_t src_step, int src_rows, int src_cols, float *dst, size_t dst_step, void *stream);
/* createVMap(const Intr&, const MapArr& depth, MapArr& vmap)                 Map.cu:8-29, 73-86 */
int xs_create_vmap(const float *intr4, const float *depth, size_t depth_step, int rows, int cols, float *vmap, size_t vmap_step,
                   void *stream);
/* createNMap(const MapArr& vmap, MapArr& nmap); rows = rows of one plane     Map.cu:32-70, 89-102 */
int xs_create_nmap(const float *vmap, float *nmap, size_t map_step, int rows, int cols, void *stream);
/* createVMap + createNMap of every pyramid level (1..3) in one launch — the six calls SurfaceMeasure makes
 * per frame (KinectFusionReconstruction.cpp:290-296); same values.  intr4s: levels x {fx, fy, cx, cy}
 * (already divided per level); level l is (rows0 >> l) x (cols0 >> l); pointer / pitch arrays per level. */
int xs_create_vnmaps(int levels, const float *intr4s, const float *const *depths, const size_t *depth_steps, int rows0, int cols0,
                     float *const *vmaps, float *const *nmaps, const size_t *map_steps, void *stream);
/* xs_create_vnmaps that also writes the real parts of both maps as float planes (vreal[l] / nreal[l]: 3 x rows(l) rows of cols(l)
 * floats, pitch real_steps[l] bytes, NaN sentinel in the x plane).  The current-frame maps come from a real depth image, so their
 * imaginary parts are zeros, and the ICP reduction can read these planes instead (xs_icp_accumulate_real /
 * xs_icp_accumulate_posted_real: half the bytes of its current-frame reads).  The three arrays are all given or all NULL. */
int xs_create_vnmaps_real(int levels, const float *intr4s, const float *const *depths, const size_t *depth_steps, int rows0, int cols0,
                          float *const *vmaps, float *const *nmaps, const size_t *map_steps, float *const *vreal, float *const *nreal,
                          const size_t *real_steps, void *stream);
/* resizeVMap / resizeNMap(const MapArr& in, MapArr& out); src_rows = rows of one input plane
 *                                                                            Map.cu:105-152, 233-259 */
int xs_resize_vmap(const float *in, size_t in_step, int src_rows, int src_cols, float *out, size_t out_step, void *stream);
int xs_resize_nmap(const float *in, size_t in_step, int src_rows, int src_cols, float *out, size_t out_step, void *stream);
/* Levels 1 and 2 of both model maps in one launch (what the orchestrator does with two resizeVMap and
 * two resizeNMap calls per frame, KinectFusionReconstruction.cpp:272-277); same values as the four
 * separate calls.  rows0 / cols0: one plane of the level-0 maps. */
int xs_resize_pyramid(const float *vmap0, const float *nmap0, size_t in_step, int rows0, int cols0, float *vmap1, float *nmap1,
                      size_t mid_step, float *vmap2, float *nmap2, size_t out_step, void *stream);
/* (xs_resize_pyramid_ex, below: the same with a completion event riding on the dispatch) */

/* ---- Raycast ------------------------------------------------------------------------------ */
/* raycast(const Intr&, const MatS33& Rc2v, const devComplex3& tc2v, const MatS33& Rv2w,
 *         const devComplex3& tv2w, float tranc_dist, const int3& res, float voxel_size,
 *         const PtrStep<float>& value, const PtrStep<float>& grad, MapArr& vmap, MapArr& nmap)
 *                                                  RayCaster.h:21-25, RayCaster.cu:197-368
 * rows / cols: one map plane.  hits_dev: optional device counter of pixels given a vertex.
 * workspace: optional rows*cols device floats (march kernel + crossing kernel instead of one). */
int xs_raycast(const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
               float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step,
               float *vmap, float *nmap, size_t map_step, int rows, int cols, unsigned long long *hits_dev, float *workspace,
               void *stream);
/* (Measurement hook of bench.py, SURVEY 8(d) "Raycast: report Mrays/s and steps/ray": xs_raycast_opts.steps_dev, a device buffer of
 * rows x cols ints that xs_raycast_ex fills with each ray's march length — the iterations the reference's loop, RayCaster.cu:222-247, runs for it.) */

/* ---- The sign map: where a ray's march may start (no counterpart in the reference) ---------------------------------------------
 * RayCaster.cu:222-247 evaluates every step of every ray from t = 0.2 m.  Each event that can end that loop — a sample outside the
 * volume, a + to - crossing, a - to + crossing — needs a sample outside or a NEGATIVE voxel on one side of the step.  The sign map keeps
 * one byte per brick of 2^shift voxels a side, set once a negative value has been written into the brick (never cleared but by reset /
 * rebuild: a superset); the march (single GPU, or a rank's slab march) samples it along the ray, finds the stretch that cannot hold an event, and resumes the
 * reference's loop behind it at the float time that loop would have there (a table of its running sum) with the value it would
 * carry — the same crossing, vertex and normal bits, about a fifth of the volume reads (march kernel 48 -> 22 us on the benchmark scene).  The owner of the volume is responsible for
 * the map seeing every write: xs_integrate_scaled_ex2 marks it when xs_integrate_opts.signmap names it; after any other write into the value
 * array (a checkpoint, a host upload) call xs_signmap_rebuild, after xs_init_volume call xs_signmap_reset.
 *   xs_raycast_signmap_shift   the smallest brick shift the march can use for these intrinsics, voxel size and truncation distance — the
 *                        finest map, measured fastest — or 0 if none (the bricks must outgrow a wave's pixel tile at 5 m; the march at most
 *                        320 steps long)
 *   xs_signmap_bytes     size of the device buffer for a resolution and brick shift (2..6; 3 = 8^3 voxels), 0 if invalid
 *   xs_signmap_reset     empty map + the time table for tranc_dist (time step 0.8 * tranc_dist, RayCaster.cu:350)
 *   xs_signmap_rebuild   reset, then mark every brick of `value` that holds a negative voxel
 *   xs_integrate_opts.signmap  the map an xs_integrate_scaled_ex2 call marks (slab launches mark the bricks of their own planes; NULL = none).  EVERY
 *                              integrate call on a volume that has a map must name it: the streamed planes of a later call do not re-mark
 *                              what an unmarked earlier call wrote
 *   xs_raycast_opts.signmap / signmap_shift / signmap_tranc_dist   the map an xs_raycast_ex (with a workspace) / xs_raycast_slab_ex call marches
 *                              by — a rank of a sharded volume passes the map its own integrate calls (owned slab + halo) marked; it must
 *                              have been reset for the same tranc_dist, else the call refuses; NULL = march from t = 0.2 */
int xs_raycast_signmap_shift(const float *intr4, float voxel_size, float tranc_dist);
size_t xs_signmap_bytes(const int *res, int shift);
int xs_signmap_reset(void *signmap, const int *res, int shift, float tranc_dist, void *stream);
int xs_signmap_rebuild(void *signmap, const int *res, int shift, float tranc_dist, const float *value, size_t vol_step, void *stream);
int xs_signmap_rebuild_slab(void *signmap, const int *res, int shift, float tranc_dist, const float *value, size_t vol_step, int zs0, int zs1,
                            void *stream);   /* one rank's storage of a z-sharded volume: value holds planes [zs0, zs1) */

/* The one-launch form of xs_raycast (workspace + sign map) can build the model-map pyramid too — levels 1 and 2 of the vertex and of the
 * normal map, the values xs_resize_pyramid writes (resizeVMap / resizeNMap twice, Map.h:46-54): every workgroup halves its own pixel tile
 * twice, so the frame's tail loses a launch.  xs_raycast_opts.pyr_* name the four maps (NULLs: none); .pyramid_built tells whether the call
 * built them (0: launch xs_resize_pyramid as before); .completion_event rides on that launch's dispatch (its completion), or NULL. */

/* Slab form for a z-sharded volume (the reference is single-GPU; per-ray semantics are those of
 * RayCaster.cu:197-310).  value / grad hold planes [zs0, zs1) = owned slab + halo (6 planes);
 * only march steps whose sample voxel lies in the owned planes [z0, z1) are evaluated.
 * keys_dev[rows*cols]: per pixel (step << 1 | no_vertex) of the first event among those steps, or
 * INT_MAX.  vmap / nmap: this rank's vertex / normal for its own event, zeros elsewhere.
 * Protocol: keys -> all-reduce(min) -> xs_raycast_compose_mask -> all-reduce(sum) of the maps as
 * int32 -> xs_raycast_compose_finish. */
int xs_raycast_slab(const float *intr4, const float *Rc2v18, const float *tc2v6, const float *Rv2w18, const float *tv2w6,
                    float tranc_dist, const int *res, float voxel_size, const float *value, const float *grad, size_t vol_step,
                    int zs0, int zs1, int z0, int z1, float *vmap, float *nmap, size_t map_step, int rows, int cols, int *keys_dev,
                    void *stream);
int xs_raycast_compose_mask(const int *own_keys_dev, const int *min_keys_dev, float *vmap, float *nmap, size_t map_step, int rows,
                            int cols, void *stream);
int xs_raycast_compose_finish(const int *min_keys_dev, float *vmap, float *nmap, size_t map_step, int rows, int cols,
                              unsigned long long *hits_dev, void *stream);
/* The composite without the sum of the maps (round 4): xs_raycast_compose_pack packs the pixels this rank owns with a vertex (own key ==
 * min key) into entries of xs_raycast_compose_entry_bytes() = 52 bytes {pixel index, vertex (3 complex), normal (3 complex)} and advances
 * *count_dev (zeroed by the caller; room for rows * cols entries) by their number; the caller gathers the ranks' packs (variable sizes)
 * and hands all of them to xs_raycast_compose_scatter, which writes them into the maps; then xs_raycast_compose_finish as before.  Per
 * rank and frame a ring all-reduce of the maps moves 2 (N - 1) / N x 14.7 MB, the gathered packs (N - 1) / N x 52 B x hits: half. */
size_t xs_raycast_compose_entry_bytes(void);
int xs_raycast_compose_pack(const int *own_keys_dev, const int *min_keys_dev, const float *vmap, const float *nmap, size_t map_step, int rows, int cols,
                            void *entries_dev, int *count_dev, void *stream);
int xs_raycast_compose_scatter(const void *entries_dev, long n, float *vmap, float *nmap, size_t map_step, int rows, int cols, void *stream);

/* First-order CSFD Gauss-Newton terms of ComputeLocalTsdfHessianKernel's residual for six seeded poses in one
 * pass over the volume (BASELINE config 5; the reference has only the single-direction kernels above).
 * Rv2c108 / tv2c36: six MatS33 / devComplex3, pose k carrying i*h on degree of freedom k (equal real parts).
 * out29_dev: sum d_j d_k for j <= k (21, row-major upper triangle), sum d_k r (6), sum r^2, count, with
 * d_k = Im(error_k) = h * dr/dtheta_k and r = Re(error_0), over voxels with gt != 0, |gt| <= 0.95 that pass the
 * kernel's gates for all six poses.  Other arguments as xs_compute_local_tsdf_hessian.  No synchronisation.
 * workspace: first 256 bytes ZERO (xs_tsdf_reduce_workspace_init).  Otherwise no workgroup is elected last and nothing
 * is published: out29_dev keeps its old contents and the call still returns 0 (the orchestrator's wait reports such a
 * launch as an error instead of spinning). */
int xs_tsdf_gauss_newton_terms(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, const int *res,
                               float voxel_size, const float *Rv2c108, const float *tv2c36, float tranc_dist, const float *gt, int z0, int z1,
                               void *workspace, double *out29_dev, void *stream);
/* ... with the loop protocol the ICP iterations have (round 6): opts NULL = plain xs_tsdf_gauss_newton_terms.  The same workspace contract: first
 * 256 bytes ZERO (xs_tsdf_reduce_workspace_init), otherwise nothing is published — neither out29_dev nor publish_host's word; the orchestrator's
 * wait then sees the stream drain without the word and reports that as an error instead of spinning.
 *   publish_host / publish_seq   host-coherent pinned memory of xs_gn_publish_bytes() bytes (hipHostMalloc, coherent + mapped): the launch's last
 *                                workgroup stores the 29 sums there and then the 64-bit word [32] = publish_seq; the host spins on that word
 *                                instead of hipMemcpyAsync + hipStreamSynchronize.  Use a different number for every launch on a buffer.
 *   pose_mailbox / mailbox_seq   with Rv2c108 = tv2c36 = NULL: the launch is enqueued BEFORE its poses exist (the host is still solving the
 *                                previous pass) and takes them from the mailbox — xs_icp_mailbox_alloc memory, written by xs_gn_post_poses with
 *                                the same number.  xs_gn_post_poses(..., cmd = 1) makes the launch leave; so does a pose that never comes (about a
 *                                second): nothing is summed, out29_dev is not written and the publish word becomes publish_seq | 1 << 63 — written by
 *                                the launch's LAST workgroup like the sums would be (every workgroup arrives whatever it did, so a launch publishes
 *                                exactly one record and leaves the workspace's ticket at zero; a launch of which only some workgroups saw their poses
 *                                before the deadline counts as left).  A posted launch also leaves, in
 *                                double [30] of the record, the 100 MHz ticks its first workgroup waited for the poses (from resident to poses seen:
 *                                the host's side of the loop as the device sees it). */
typedef struct xs_gn_opts {
    unsigned struct_bytes;            /* sizeof(xs_gn_opts) */
    unsigned mailbox_seq;
    const void *pose_mailbox;
    double *publish_host;
    unsigned long long publish_seq;
} xs_gn_opts;
int xs_tsdf_gauss_newton_terms_ex(const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4, const int *res,
                                  float voxel_size, const float *Rv2c108, const float *tv2c36, float tranc_dist, const float *gt, int z0, int z1,
                                  void *workspace, double *out29_dev, const xs_gn_opts *opts, void *stream);
size_t xs_gn_publish_bytes(void);     /* 33 doubles */
size_t xs_gn_mailbox_bytes(void);     /* six pose mailboxes in a row (xs_icp_mailbox_alloc's 4096 bytes hold them) */
/* host: the six seeded poses (or cmd 1 = leave) for the launch polling mailbox_host for mailbox_seq */
void xs_gn_post_poses(void *mailbox_host, const float *Rv2c108, const float *tv2c36, unsigned mailbox_seq, int cmd);
/* shard mode: the n <= 32 sums as they stand in device memory behind the stream's all-reduce, published like the kernel's own (word [32] = seq) */
int xs_gn_publish_sums(const double *sums_dev, int n, double *publish_host, unsigned long long seq, void *stream);

/* ---- band index of a fixed map: batched Gauss-Newton passes for relocalisation (xs_band.hip) ------------------
 * xs_tsdf_gauss_newton_terms scans the whole slab on every pass to find its band voxels (gt != 0, |gt| <= 0.95).  The band depends on gt
 * alone, so for a map that does not change it can be found once: xs_tsdf_band_build records the band voxels of the slab [z0, z1) of gt in
 * the order the Gauss-Newton kernel's walk deals them to its lanes — per wave segment (workgroup b, wave w), entry 64 k + lane for the
 * lane's k-th take — and xs_tsdf_gauss_newton_terms_band replays that order for up to XS_BAND_MAX_FRAMES query frames per launch.  Frame
 * f's 29 sums are bit-identical to those of xs_tsdf_gauss_newton_terms for the same depth, poses and gt (same tiling: the build reads gt at
 * the address the dense pass would be given, whose 16-byte alignment picks the walk), whatever the other frames of the launch are. */
#define XS_BAND_MAX_FRAMES 32
#define XS_BAND_OVER_CAPACITY (-3)
typedef struct xs_band_index {
    /* the caller's buffers */
    unsigned long long *keys;       /* capacity entries: x | y << 21 | z << 42 (global voxel coordinates) */
    float *values;                  /* capacity entries: gt at the key, bit for bit */
    long long capacity;
    long long *segs;                /* device, xs_tsdf_band_segs_bytes(res, z0, z1): [0, 4 nblocks) offsets, [4 nblocks, 8 nblocks) lengths of the
                                       wave segments (segment 4 b + w: workgroup b, wave w of the dense pass) */
    /* filled by the build */
    long long count;                /* band voxels */
    int nblocks;                    /* workgroups of the dense pass over this slab */
    int res[3], z0, z1;
} xs_band_index;
size_t xs_tsdf_band_segs_bytes(const int *res, int z0, int z1);
/* Two walks over the slab: lengths, then (their exclusive scan on the host) keys and values.  index->count and the other filled fields are
 * always set; if count > capacity the call returns XS_BAND_OVER_CAPACITY and writes neither keys nor values (count-then-fill: capacity 0 and
 * NULL arrays count; segs is written either way).  Synchronises the stream. */
int xs_tsdf_band_build(const float *gt, const int *res, int z0, int z1, xs_band_index *index, void *stream);
/* workspace of xs_tsdf_gauss_newton_terms_band for up to `frames` frames: per-frame arrival tickets in its first 256 bytes, the poses, the
 * records.  Zero the first 256 bytes ONCE after allocation (xs_tsdf_reduce_workspace_init does it): every launch leaves each frame's ticket at
 * zero again.  One launch at a time per workspace; after a launch that did not complete (a device fault), zero them again. */
size_t xs_tsdf_band_workspace_bytes(int frames);
/* The six-pose Gauss-Newton terms of `frames` (1 .. XS_BAND_MAX_FRAMES) query frames over a built index: frame f's depth is
 * depth_scaled[f] (host array of device pointers; all frames rows x cols with one step), its six seeded poses Rv2c108xF + 108 f /
 * tv2c36xF + 36 f (the layout of xs_tsdf_gauss_newton_terms), its 29 sums out29xF_dev + 29 f.  No synchronisation. */
int xs_tsdf_gauss_newton_terms_band(int frames, const float *const *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                                    float voxel_size, const float *Rv2c108xF, const float *tv2c36xF, float tranc_dist, const xs_band_index *index,
                                    void *workspace, double *out29xF_dev, void *stream);
/* ---- the exact 6 x 6 pose Hessian of the map-alignment loss in one pass over the index ----
 * Per query frame 21 dual-complex poses in the layout of xs_compute_local_tsdf_hessian (MatD33 36 floats + devDComplex3 12 floats), one per
 * pair of se(3) generators (a, b), a <= b, in the order (0,0), (0,1), ..., (5,5): real part v2c (the same bits in all 21), eps1 = -h v2c G_a,
 * eps2 = -h v2c G_b, eps1 eps2 = h^2 v2c (G_a G_b + G_b G_a) / 2.  Frame f's 29 sums land at out29xF_dev + 29 f:
 *   [0, 21)  sum loss_ab.hessian(), row-major upper triangle (/ h^2: d2L / dtheta_a dtheta_b of L(inverse(se3Exp(theta) c2v)) at 0)
 *   [21, 27) sum loss_aa.grad() (/ h: dL / dtheta_a)        [27] sum r^2 (pair (0,0))        [28] count
 * with the per-voxel loss of xs_compute_local_tsdf_hessian.  A band voxel counts only if all 21 evaluations keep it.  The entries of the
 * index are dealt out in chunks of 64 (not in the dense walk's segments), and the sums are folded in a fixed order: two launches on the same
 * inputs give the same bits, and frame f's sums do not depend on `frames`, on f or on the other frames.
 * Workspace: xs_tsdf_pose_hessian_workspace_bytes(frames) bytes (0 for frames outside 1 .. XS_BAND_MAX_FRAMES), the first 256 zeroed ONCE
 * after allocation (xs_tsdf_reduce_workspace_init); every launch leaves them zero.  One launch at a time per workspace.  No synchronisation. */
size_t xs_tsdf_pose_hessian_workspace_bytes(int frames);
int xs_tsdf_pose_hessian_band(int frames, const float *const *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                              float voxel_size, const float *Rv2c36x21xF, const float *tv2c12x21xF, float tranc_dist, const xs_band_index *index,
                              void *workspace, double *out29xF_dev, void *stream);
/* ---- the real-valued alignment loss of one depth frame at many poses in one pass over the index ----
 * `poses` (1 .. XS_SCORE_MAX_POSES) real volume-to-camera poses, host arrays Rv2c9xP + 9 p / tv2c3xP + 3 p in the layout of
 * xs_compute_local_tsdf_loss.  Pose p's two doubles land at out2xP_dev + 2 p: {sum loss, count}, the shape of that kernel's out2.  A band
 * voxel's float loss and its keep / drop decision are those of xs_compute_local_tsdf_loss, so pose p's count EQUALS the count that call
 * returns for the pose on the dense gt the index was built from, and its sum adds the same float terms: each 64-entry chunk of the index in a
 * six-level pairwise float tree across the wave, everything after that in double — |sum - dense sum| <= 8 * 2^-24 * dense sum.  The order is a
 * function of the index's count alone: two launches on the same inputs give the same bits, and pose p's two numbers do not depend on
 * `poses`, on p or on the other poses.  No floating-point atomics.  An index with count 0 yields zeros.
 * Workspace: xs_tsdf_score_poses_workspace_bytes(poses) bytes (0 for poses outside 1 .. XS_SCORE_MAX_POSES): one arrival ticket per tile of
 * 64 poses in its first 256 bytes, the poses, the records.  Zero the first 256 bytes ONCE after allocation (xs_tsdf_reduce_workspace_init);
 * every launch leaves each ticket at zero again.  One launch at a time per workspace; after a launch that did not complete (a device
 * fault), zero them again.  No synchronisation. */
#define XS_SCORE_MAX_POSES 4096
size_t xs_tsdf_score_poses_workspace_bytes(int poses);
int xs_tsdf_score_poses_band(int poses, const float *depth_scaled, size_t scaled_step, int rows, int cols, const float *intr4,
                             float voxel_size, const float *Rv2c9xP, const float *tv2c3xP, float tranc_dist,
                             const xs_band_index *index, void *workspace, double *out2xP_dev, void *stream);

/* ---- what a hypothetical camera would see of the map: next best view (xs_view.hip) ----------------------------
 * No counterpart in the reference.  The OBSERVATION GRID condenses the value and weight volumes into two bits per voxel:
 *   0 UNKNOWN  weight < min_weight        1 FREE  weight >= min_weight and value >= 0        2 OCCUPIED  weight >= min_weight and value < 0
 * (min_weight below 1 means 1, as in xs_mesh_opts; -0.0f is FREE).  The integrate step leaves weight 0 exactly where nothing was fused and
 * writes tsdf = 1 with weight >= 1 into the free space in front of a surface, so the grid is a function of the stored volumes alone.
 * Layout (the library's own business; use xs_view_grid_expand to read it): one 16-byte word per brick of 4 x 4 x 4 voxels, bricks in x, y,
 * z order, two bits per voxel at bit 2 (lx + 4 ly + 16 lz); bricks that overhang the volume are padded and the padding is never read as a
 * state.  Behind the bricks the buffer holds the staging area xs_score_views copies a launch's poses into.
 * xs_view_grid_bytes: the buffer's size (16-byte aligned device memory), 0 for a resolution with a non-positive axis.  Host only.
 * xs_view_grid_build: the whole volume (value and weight with one row pitch vol_step, rows in (z * Y + y) order); reads 8 bytes per voxel
 * once, by 16-byte loads where the pointers and the pitch are 16-byte aligned.  No synchronisation.
 * xs_view_grid_expand: one byte per voxel, states_dev[(z * Y + y) * X + x]: tests and viewers.  No synchronisation. */
size_t xs_view_grid_bytes(const int *res);
int xs_view_grid_build(const float *value, const int *weight, size_t vol_step, const int *res, int min_weight, void *grid, void *stream);
int xs_view_grid_expand(const void *grid, const int *res, unsigned char *states_dev, void *stream);
/* xs_score_views: `poses` (1 .. XS_VIEW_MAX_POSES) real camera-to-volume poses, host arrays Rc2v9xP + 9 p (row-major) / tc2v3xP + 3 p, each
 * casting a lattice of rays_x x rays_y rays of a rows x cols camera with intrinsics intr4 through the grid, all in one launch.  The call
 * zeroes out4xP_dev[4 p .. 4 p + 3] on the stream and the launch leaves there {unknown, free, hits, frontier} of pose p:
 *   ray (i, j):  u = (float(i) + 0.5f) * (float(cols) / float(rays_x)),  v = (float(j) + 0.5f) * (float(rows) / float(rays_y)),
 *                dx = (u - cx) / fx,  dy = (v - cy) / fy,  d[c] = (R[c][0] * dx + R[c][1] * dy) + R[c][2]   (not normalised: t is depth along
 *                the camera's z)
 *   sample k = 0, 1, ... while t_k < t_far:  t_k = t_near + float(k) * step (no running sum),  p[c] = tc2v[c] + t_k * d[c],
 *                voxel floor(p[c] / voxel_size) by an IEEE divide, as in the raycast
 *   a sample whose voxel lies outside [0, res) counts nothing and does not end the ray; otherwise its state counts: UNKNOWN adds 1 to
 *   `unknown`, and 1 to `frontier` if the ray's previous in-volume sample was FREE; FREE adds 1 to `free`; OCCUPIED adds 1 to `hits` and ends
 *   the ray.
 * Every operation is a separate IEEE float operation in this order (the library is built -ffp-contract=off) and the counters are integers,
 * added by integer atomics: the result is a pure function of the inputs — a float32 model on the host reproduces it exactly, two launches
 * give the same bits, and pose p's four numbers do not depend on `poses`, on p or on the other poses.  No floating-point atomics.
 * hipErrorInvalidValue, with nothing launched and out4xP_dev untouched: poses outside 1 .. XS_VIEW_MAX_POSES; a lattice dimension below 1 or
 * above cols / rows; step < 0 (or, after the default, not positive); t_far <= t_near; more than 4096 samples per ray; rays_x * rays_y *
 * samples >= 2^32.  One launch at a time per grid (the poses' staging area).  No synchronisation. */
#define XS_VIEW_MAX_POSES 4096
typedef struct xs_view_opts {
    unsigned struct_bytes;     /* sizeof(xs_view_opts) */
    int rays_x, rays_y;        /* the ray lattice; 0, 0 = 80 x 60 */
    float t_near, t_far;       /* depth range along the camera's z; 0, 0 = 0.2, 5.0 (xs_scale_depth's valid range) */
    float step;                /* depth increment per sample; 0 = voxel_size */
} xs_view_opts;
int xs_score_views(int poses, const float *Rc2v9xP, const float *tc2v3xP, const float *intr4, int rows, int cols, const int *res,
                   float voxel_size, const void *grid, const xs_view_opts *opts, unsigned *out4xP_dev, void *stream);

/* ---- clearance and reachability from the observation grid (xs_reach.hip) ----------------------------------------
 * No counterpart in the reference.  Integer arithmetic on the grid's states throughout: every result is a pure function of the inputs, two
 * runs give equal bytes, no floating-point atomics.  `grid` is the observation grid as xs_view_grid_build leaves it; the volumes are not read.
 * CLEARANCE FIELD.  Obstacles: the OCCUPIED voxels; with unknown_blocks = 1 also the UNKNOWN voxels and every voxel position outside
 * [0, res) (outside the volume nothing is known).  The padding bits of overhanging bricks are never read as a state.
 *   field[(z * Y + y) * X + x] (uint16, dense) = min(d2, R * R), R = max_radius in voxels (1 .. XS_CLEARANCE_MAX_RADIUS), d2 the least
 *   dx * dx + dy * dy + dz * dz from the voxel to an obstacle voxel: 0 on obstacles, R * R everywhere when there is no obstacle at all.
 * Three plain launches on the stream (a distance along x per voxel, then a windowed minimum of f(j) + (j - i)^2 over |j - i| <= R along y
 * and along z; exact under the cap, since an obstacle within distance R lies in the R-cube and every other candidate is above R * R);
 * the intermediates live in `workspace` (xs_clearance_workspace_bytes: three bytes per voxel; 256-byte aligned device memory).
 * xs_clearance_bytes: the field's size, 2 bytes per voxel.  Both sizes are 0 for a resolution with a non-positive axis, or with Y or Z above
 * 65535.  Host only.
 * xs_clearance_build: hipErrorInvalidValue, with nothing launched and `field` untouched, for max_radius outside 1 .. 255, unknown_blocks
 * other than 0 or 1, such a resolution, or a null pointer.  No synchronisation. */
#define XS_CLEARANCE_MAX_RADIUS 255
size_t xs_clearance_bytes(const int *res);
size_t xs_clearance_workspace_bytes(const int *res);
int xs_clearance_build(const void *grid, const int *res, int max_radius, int unknown_blocks, void *workspace, unsigned short *field_dev, void *stream);
/* REACHABILITY.  A voxel is PASSABLE iff its state is FREE and field >= r2 (r2 an integer, 1 .. R * R of the field the caller built: a body
 * of squared radius r2 voxels fits there).  REACHED is the union of the 6-connected (face-neighbour) components of the passable set that hold
 * a seed.  `reach` (xs_reach_bytes(res) bytes, 8-byte aligned device memory) holds both as one 64-bit mask per brick of 4 x 4 x 4 voxels,
 * bricks in the grid's order, voxel (lx, ly, lz) at bit lx + 4 ly + 16 lz, overhang bits clear: the reached words first, the passable
 * words behind them, then the flood's control words.
 * xs_reach_passable: the passable words alone (what a start is snapped over before the flood).  No synchronisation.
 * xs_reach_flood: `seeds` (1 .. XS_REACH_MAX_SEEDS) integer voxels, host array seeds3xN + 3 k = (x, y, z).  A seed outside the volume or not
 * passable contributes nothing (no error); duplicates are harmless.  Builds the passable words, clears the reached words, sets the seeds'
 * bits and runs rounds as plain launches: a lane owns one brick word, grows it to its in-brick fixpoint, pulls the facing bits of the six
 * neighbouring words, writes its own word only and sets a `changed` word with a plain store if it grew.  Words only gain bits, so in-place
 * update needs no atomics and the result does not depend on scheduling (the number of rounds may).  The host reads the changed words back
 * after each batch of rounds and stops after the first round that changed nothing: THE CALL SYNCHRONISES THE STREAM.  *rounds_out (optional)
 * receives the number of rounds up to and including that one.
 * xs_reach_expand: out_dev[(z * Y + y) * X + x] = 0 or 1 from the reached words (passable = 0) or the passable words (passable = 1): tests
 * and viewers.  No synchronisation.
 * hipErrorInvalidValue with nothing written: seeds outside 1 .. 64, r2 < 1 (or above 255 * 255), a bad resolution, null pointers. */
#define XS_REACH_MAX_SEEDS 64
size_t xs_reach_bytes(const int *res);
int xs_reach_passable(const void *grid, const unsigned short *field_dev, const int *res, int r2, void *reach, void *stream);
int xs_reach_flood(const void *grid, const unsigned short *field_dev, const int *res, int r2, const int *seeds3xN, int seeds, void *reach,
                   int *rounds_out, void *stream);
int xs_reach_expand(const void *reach, const int *res, int passable, unsigned char *out_dev, void *stream);
/* POINT QUERY.  n >= 1 points in volume coordinates (float32 metres, device array points3xN_dev + 3 i).  The voxel s of a point is
 * floor(p[c] / voxel_size) per axis by an IEEE divide, as in the raycast and xs_score_views, tested against [0, res) before anything is
 * fetched (a NaN is outside).  Per point: reachable_dev[i] (0 or 1) and clear2_dev[i] (a field value):
 *   outside the volume                               (0, 0)
 *   s is in the mask                                 (1, field[s])
 *   otherwise, snap > 0 (voxels, <= XS_REACH_MAX_SNAP): the voxel v of the mask with |v - s|_inf <= snap that has the least |v - s|^2,
 *                                                    ties to the lowest linear index (z * Y + y) * X + x:   (1, field[v])
 *   no such voxel, or snap = 0                       (0, field[s])
 * The mask is the reached words of `reach`, or with over_passable = 1 the passable words.  voxel3xN_dev (optional, int32) receives the
 * answering voxel (s or v), (-1, -1, -1) where the answer is 0.  hipErrorInvalidValue with nothing written: n < 1, snap outside 0 .. 16,
 * voxel_size not positive, a bad resolution, null pointers.  No synchronisation. */
#define XS_REACH_MAX_SNAP 16
int xs_reach_query(int n, const float *points3xN_dev, const int *res, float voxel_size, const void *reach, int over_passable,
                   const unsigned short *field_dev, int snap, unsigned char *reachable_dev, unsigned short *clear2_dev, int *voxel3xN_dev,
                   void *stream);

/* ---- travel cost and shortest collision-free path over the reached set (xs_travel.hip) --------------------------
 * No counterpart in the reference.  Integer arithmetic throughout, no atomics: every result is a pure function of the inputs and two runs
 * give equal bytes.  DOMAIN: the REACHED voxels, read from the reached words of `reach` as xs_reach_flood leaves them.
 * MOVES: the 26 neighbour offsets o = (dx, dy, dz) != 0, components in {-1, 0, 1}; the cost w(o) is 3, 4 or 5 for one, two or three non-zero
 * components (the <3, 4, 5> chamfer metric: a unit is a third of a voxel edge).  v -> v + o is ALLOWED iff v + o is in the domain and so is
 * every v + o', o' being o with a non-empty proper subset of its non-zero components set to zero (the 2 face neighbours of an edge move, the
 * 6 face and edge neighbours of a corner move): the body never squeezes between two obstacle voxels that touch diagonally.  The rule is
 * symmetric in v and v + o, and an allowed diagonal move implies a 6-connected detour.
 * FIELD.  travel[(z * Y + y) * X + x] (uint16, dense; xs_travel_bytes(res): 2 bytes per voxel, 0 for a bad resolution) is 0 at every seed
 * that is in the domain, elsewhere the least sum of w over paths of allowed moves from a seed if that sum is <= limit (0 .. XS_TRAVEL_MAX;
 * 0: the seeds only), and XS_TRAVEL_NONE otherwise.  Sums are formed in 32 bits and a candidate above the limit is dropped, never stored:
 * the field is the unique fixpoint of d[v] = min(d[v], d[u] + w) under that cap.
 * xs_travel_build: `seeds` (1 .. XS_REACH_MAX_SEEDS) integer voxels, host array seeds3xN + 3 k = (x, y, z); a seed outside the volume or
 * outside the domain contributes nothing.  Fills the field with 0xFF, writes the seeds' zeros and runs rounds as plain launches: a
 * workgroup owns a tile of 8 x 8 x 8 voxels (2 x 2 x 2 bricks), returns at once if none of its reached words has a bit, otherwise holds the
 * tile with a one-voxel apron in LDS, relaxes it there until nothing in the tile changes, writes back its own voxels that fell and sets the
 * round's `changed` word with a plain store.  Aprons are re-read from global memory every round; a stale value delays a distance by a
 * round and never invents one, so the result does not depend on scheduling (the number of rounds may).  The host reads the changed words
 * (in `workspace`: xs_travel_workspace_bytes() of device memory, 4-byte aligned, not the reach buffer) after each batch of rounds and
 * stops after the first round that changed nothing: THE CALL SYNCHRONISES THE STREAM.  *rounds_out (optional) receives the number of
 * rounds up to and including that one.
 * xs_travel_query: n >= 1 integer voxels (int32 device array voxel3xN_dev + 3 i = (x, y, z), e.g. the answering voxels of xs_reach_query):
 * out_dev[i] = travel[v], XS_TRAVEL_NONE outside the volume.  No synchronisation.
 * xs_travel_path: n targets (1 .. XS_TRAVEL_MAX_TARGETS, int32 device array), one lane each.  From a target t with travel[t] != NONE: while
 * travel[v] != 0, step to v + o for the allowed move with travel[v + o] + w(o) = travel[v] that has the lowest index k = (dz + 1) * 9 +
 * (dy + 1) * 3 + (dx + 1) (one exists at a fixpoint).  The path is the voxels visited, t first and the seed last; path3_dev[(i * capacity
 * + s) * 3 ..] receives voxel s of target i for s < min(length, capacity), slots beyond that are untouched; len_dev[i] receives the full
 * length even when it exceeds capacity: 1 when t is a seed, 0 when travel[t] = NONE or t is outside the volume.  `limit` (that of the
 * build) only bounds the walk's trip count, at limit / 3 + 2, so that a corrupt field cannot spin it.  No synchronisation.
 * hipErrorInvalidValue with nothing launched and the outputs untouched: null pointers, a bad resolution, seeds outside 1 .. 64, limit
 * outside 0 .. 65534, n outside its range, capacity < 1. */
#define XS_TRAVEL_NONE 65535
#define XS_TRAVEL_MAX 65534
#define XS_TRAVEL_MAX_TARGETS 64
size_t xs_travel_bytes(const int *res);
size_t xs_travel_workspace_bytes(void);
int xs_travel_build(const void *reach, const int *res, const int *seeds3xN, int seeds, int limit, unsigned short *travel_dev, void *workspace,
                    int *rounds_out, void *stream);
int xs_travel_query(int n, const int *voxel3xN_dev, const int *res, const unsigned short *travel_dev, unsigned short *out_dev, void *stream);
int xs_travel_path(int n, const int *target3xN_dev, const int *res, const void *reach, const unsigned short *travel_dev, int limit, int capacity,
                   int *path3_dev, int *len_dev, void *stream);

/* ---- frontier voxels, their clusters and one record per cluster (xs_frontier.hip) -------------------------------
 * No counterpart in the reference.  Integer arithmetic on the grid's states throughout, no floating-point atomics; the integer atomics used
 * (add, min, max) give results that do not depend on their order: every result is a pure function of the inputs and two runs give equal
 * bytes.  `grid` is the observation grid as xs_view_grid_build leaves it; the volumes are not read and the grid is not written.
 * RESOLUTIONS: those of the reach calls (every axis >= 1, Y and Z <= 65535, fewer than 2^31 bricks) with X * Y * Z < 2^32 - 1, so that a
 * uint32 indexes every voxel and XS_FRONTIER_NONE stays free.  For any other the three size functions return 0 and every call refuses.
 * MASK.  A voxel is FRONTIER iff its state is FREE and at least one of its six face neighbours inside the volume is UNKNOWN.  A position
 * outside [0, res) is not UNKNOWN for this purpose (an all-FREE volume has no frontier), and the padding bits of overhanging bricks are
 * never read as a state.  `mask` (xs_frontier_mask_bytes(res): 8 bytes per brick, 8-byte aligned device memory) holds one 64-bit word per
 * brick of 4 x 4 x 4 voxels in the reach buffer's layout: bricks in the grid's order, voxel (lx, ly, lz) at bit lx + 4 ly + 16 lz, overhang
 * bits clear.  xs_frontier_mask: one plain launch, a lane per brick.  No synchronisation.
 * xs_frontier_expand: out_dev[(z * Y + y) * X + x] = 0 or 1 from the mask: tests and viewers.  No synchronisation.
 * LABELS.  labels[(z * Y + y) * X + x] (uint32, dense; xs_frontier_label_bytes(res): 4 bytes per voxel) is XS_FRONTIER_NONE on a voxel that
 * is no frontier voxel and otherwise the lowest linear index (z * Y + y) * X + x among the voxels of its CLUSTER.  Two frontier voxels are
 * joined iff they differ by at most 1 on every axis (26-adjacency) and lie in the same CELL; the clusters are the connected components of
 * that relation.  Cells are cubes of `cell` voxels aligned to the origin, cell (x / cell, y / cell, z / cell); cell = 0: one cell, the whole
 * volume; otherwise a multiple of 8 in 8 .. 65528.
 * xs_frontier_label: sets every voxel's label to its own index or NONE and runs rounds as plain launches: a workgroup owns a tile of
 * 8 x 8 x 8 voxels (8 divides cell, so a tile lies in one cell), returns at once if none of its eight mask words has a bit, otherwise holds
 * the tile's labels with a one-voxel apron in LDS (NONE outside the volume and across a cell boundary), lets every frontier voxel take the
 * minimum over itself and its 26 neighbours until nothing in the tile changes, writes back its own labels that fell and sets the round's
 * `changed` word with a plain store.  Labels only fall and every stored label is the index of a voxel of the same cluster; aprons are
 * re-read from global memory every round, a stale value delays a merge by a round and never invents one, so the result does not depend on
 * scheduling (the number of rounds may).  The host reads the changed words (in `workspace`: at least xs_frontier_workspace_bytes(res, 0)
 * bytes of device memory, 8-byte aligned) after each batch of rounds and stops after the first round that changed nothing: THE CALL
 * SYNCHRONISES THE STREAM.  *rounds_out (optional) receives the number of rounds up to and including that one.
 * RECORDS.  One record of XS_FRONTIER_RECORD_WORDS = 8 uint64 per cluster, in ascending label order:
 *   {label, count, sum of x, sum of y, sum of z, min packed as x | y << 16 | z << 32, max packed likewise, 0}
 * over the cluster's voxels (min and max per axis: the bounding box).
 * xs_frontier_clusters: `labels_dev` as xs_frontier_label left them for this `mask`.  *count_dev (device) and *count_host (host, optional)
 * always receive the full number of clusters; records_dev (capacity x 8 uint64, device) is written only when that number is <= capacity,
 * and then exactly that many records: the caller retries with a larger buffer.  `workspace`: xs_frontier_workspace_bytes(res, capacity)
 * bytes.  The voxels whose label is their own index are compacted through an integer counter, the list is sorted on the host, and one
 * launch over the frontier voxels finds each voxel's record by binary search and adds with integer atomics.  Needs X <= 65535 too (the
 * packed box).  THE CALL SYNCHRONISES THE STREAM.
 * hipErrorInvalidValue, with nothing launched and the outputs untouched: null pointers (count_host and rounds_out excepted), a resolution
 * outside the set above, a bad cell, capacity < 1. */
#define XS_FRONTIER_NONE 0xFFFFFFFFu
#define XS_FRONTIER_RECORD_WORDS 8
size_t xs_frontier_mask_bytes(const int *res);
size_t xs_frontier_label_bytes(const int *res);
size_t xs_frontier_workspace_bytes(const int *res, int capacity);
int xs_frontier_mask(const void *grid, const int *res, void *mask, void *stream);
int xs_frontier_label(const void *mask, const int *res, int cell, unsigned *labels_dev, void *workspace, int *rounds_out, void *stream);
int xs_frontier_clusters(const void *mask, const unsigned *labels_dev, const int *res, int capacity, unsigned long long *records_dev,
                         unsigned *count_dev, unsigned *count_host, void *workspace, void *stream);
int xs_frontier_expand(const void *mask, const int *res, unsigned char *out_dev, void *stream);

/* ---- surface extraction (export; real-valued) ------------------------------------------------ */
size_t xs_extract_workspace_bytes(const int *res);
/* size_t extractPoints(value_volume, weight_volume, grad_volume, volume_resolution, voxel_size,
 * PtrSz<float3> output)                       ExtractPointCloud.h:19-20, ExtractPointCloud.cu:25-211
 * Zero crossings of the TSDF between axis neighbours (+x, +y, +z; both samples < 0.99, opposite signs),
 * linearly interpolated, for the voxels of planes [z0, z1), z1 <= res[2] - 1 (whole volume: 0, res[2] - 1).
 * value points at stored plane zs0 (0 for the whole volume) and holds planes up to z1 inclusive.  The weight
 * and grad volumes of the reference signature are not read there either.  points_dev: capacity x 3 floats,
 * filled in a deterministic order (workgroup, z, y, x, direction; the reference's order depends on its
 * atomics).  *count_host = min(found, capacity), the reference's return value; *found_host (optional) =
 * found.  workspace: xs_extract_workspace_bytes(res).  Synchronises the stream, as the reference does. */
int xs_extract_points(const float *value, size_t vol_step, const int *res, float voxel_size, int zs0, int z0, int z1, float *points_dev,
                      size_t capacity, void *workspace, size_t *count_host, size_t *found_host, void *stream);
/* void extractNormals(value_volume, weight_volume, grad_volume, volume_resolution, voxel_size,
 * PtrSz<float3> points, PtrSz<float3> normal)            ExtractPointCloud.h:22-23, .cu:214-362
 * Central differences of the trilinearly interpolated TSDF one voxel either side of each point, divided by
 * their squared length as in the reference; (0, 0, 0) within two voxels of the border.  value holds stored
 * planes [zs0, zs1) (whole volume: 0, res[2]).  No synchronisation. */
int xs_extract_normals(const float *value, size_t vol_step, const int *res, float voxel_size, int zs0, int zs1, const float *points_dev,
                       size_t n, float *normals_dev, void *stream);

/* ---- merging a second volume into the volume (xs_merge.hip) ----------------------------------------------------
 * No counterpart in the reference.  Both volumes use the layout of every call here: row (Y * z + y), x contiguous, one pitch (`step`,
 * `src_step`, bytes) shared by a volume's three arrays.  The destination pointers are at plane 0; only planes [z0, z1) are written.
 * *written_dev (optional, device) is INCREMENTED by the number of destination voxels written.  `workspace`:
 * xs_tsdf_merge_workspace_bytes(res, src_res) bytes of device memory (may be NULL with XS_MERGE_NO_CULL).  No synchronisation.
 *
 * Destination voxel (x, y, z); m = xform12, a 3 x 3 matrix in row-major order followed by 3 offsets, maps destination voxel indices to
 * continuous source voxel indices.  Every operation is float32, in the order written:
 *   1. g_a = ((m[3a] * float(x) + m[3a + 1] * float(y)) + m[3a + 2] * float(z)) + m[9 + a], a = 0, 1, 2.
 *   2. The voxel is skipped unless 0 <= g_a <= float(S_a - 1) on every axis (S: the source resolution; a NaN fails).  b_a = floor(g_a),
 *      f_a = g_a - float(b_a); the upper corner on axis a is NEEDED only when f_a > 0.
 *   3. The needed corners are b + d with d_a = 1 only on axes with f_a > 0: 1, 2, 4 or 8 of them.  No other corner is read (at
 *      g_a = S_a - 1 the upper corner lies outside the allocation).  ws = the smallest weight of the needed corners; the voxel is skipped
 *      unless ws >= min_weight; then ws = min(ws, max_weight).
 *   4. value and grad, each: interpolated along x, then y, then z, a stage being lo * (1.0f - f_a) + hi * f_a, and `lo` itself, with no
 *      arithmetic, on an axis with f_a == 0 (-0 stays -0): the result is s.
 *   5. wp = the destination's weight.  wp == 0: new = s.  Otherwise new = (prev * float(wp) + s * float(ws)) / float(wp + ws), for value and
 *      grad each.  weight = min(wp + ws, max_weight).  The voxel counts as written.
 * So an identity map into an empty volume is a copy bit for bit, a shift by whole voxels is a slice and an axis permutation is exact.
 * The cull (a tile of destination voxels whose source index box misses the source, or touches only bricks of 4 x 4 x 4 source voxels with no
 * weight >= min_weight, is left before any load) changes no output bit; XS_MERGE_NO_CULL switches it off: every destination voxel takes the
 * per-voxel path.  No output depends on scheduling.
 * hipErrorInvalidValue, with nothing launched: a null array, resolution or xform12 (or workspace, unless XS_MERGE_NO_CULL); an axis outside
 * 1 .. 262140; a pitch that is no multiple of 4 or shorter than a row; min_weight < 1; max_weight outside [1, 1 << 24]; an entry of xform12
 * that is not finite; an empty or reversed plane range or one outside [0, res[2]]; a source array equal to its destination counterpart. */
#define XS_MERGE_NO_CULL 1u
size_t xs_tsdf_merge_workspace_bytes(const int *dst_res, const int *src_res);
int xs_tsdf_merge(float *value, int *weight, float *grad, size_t step, const int *res, int z0, int z1, const float *src_value,
                  const int *src_weight, const float *src_grad, size_t src_step, const int *src_res, const float *xform12, int min_weight,
                  int max_weight, unsigned flags, unsigned long long *written_dev, void *workspace, void *stream);

/* ---- taking fused frames out of the volume and fusing frames with a sign (xs_reintegrate.hip) ---------------------
 * No counterpart in the reference.  One pass over planes [z0, z1) applies up to XS_REINTEGRATE_MAX_OPS observations to every voxel, each
 * with a sign.  The volume arguments are xs_integrate_scaled's: value / weight / grad at the first stored plane z0 (the whole volume: plane 0,
 * z0 = 0, z1 = res[2]), one pitch `vol_step` (bytes), z over global plane indices; only planes [z0, z1) are touched.  Every op's image is
 * rows x cols floats with the pitch `scaled_step`, as xs_scale_depth writes it (no valid depth beyond 5 m); ops may share one image.  The op
 * table is read on the host during the call and travels in the kernel's arguments: no copy to the device, no synchronisation.
 * counts4_dev (device): {removed, added, emptied, orphaned} are INCREMENTED by the numbers below, with integer atomics, one add per counter
 * and workgroup.
 *
 * The observation obs(op) at a voxel is, by definition, what xs_integrate_scaled writes into a ZEROED volume with the op's image and pose and
 * this call's intr4, voxel_size, tranc_dist and threshold: the voxel is SEEN iff that call writes it, and t = (value, grad) written there.
 * The kernel computes it with the integrate kernels' own per-voxel functions in their operation order (threshold > 0: the bilinear instance).
 * Per voxel the ops are applied in list order, each on the state the previous one left; float32, in the order written; the complex state
 * (value, grad) is divided by a real divisor component by component; w is the weight:
 *   sign = +1, seen:          new = (prev * float(w) + 1.0f * t) / float(w + 1); w = min(w + 1, max_weight): the integrate kernels' running
 *                             mean, exactly.  Counts as ADDED.
 *   sign = -1, seen, w >= 2:  new = (prev * float(w) - 1.0f * t) / float(w - 1); w = w - 1; then the real part (value) is clamped to [-1, 1] —
 *                             a mean of observations lies there, only rounding or the removal of something never added leaves it; the
 *                             imaginary part (grad) is not clamped.  Counts as REMOVED.
 *   sign = -1, seen, w == 1:  value, grad and weight become 0, the state xs_init_volume leaves.  Counts as REMOVED and as EMPTIED.
 *   sign = -1, seen, w <= 0:  nothing changes.  Counts as ORPHANED.
 *   not seen:                 nothing changes.
 * A voxel no op changes keeps its bits (a word is stored only if an op changed it); rows outside [z0, z1) and a row's padding are never
 * written.  The cull (a row of 64 x 1 x 8 voxels that an op's view frustum, padded as the integrate kernels pad it and closed at the far
 * limit of a 5 m depth, cannot see skips that op; a tile of 64 x 4 x 8 voxels no op can see is left before any load) changes no bit;
 * XS_REINTEGRATE_NO_CULL switches it off.  No output depends on scheduling.
 *
 * What removal cannot undo: once a voxel's weight has been clamped at max_weight its value is a moving average, no longer the mean of the
 * frames fused there, and taking an old frame out of it is an approximation (the frame's share has decayed, the call subtracts a full one).
 * The call cannot know this and does not refuse.  Removing an observation that was never added, or with another pose, image or parameter
 * than it was added with, is arithmetic on the same rules, not an inverse.
 *
 * hipErrorInvalidValue, with nothing launched and nothing written: `ops` outside 1 .. XS_REINTEGRATE_MAX_OPS; a sign other than +1 or -1; a
 * null ops_host, image, intr4, res, array or counts4_dev; a pose entry that is not finite; what xs_integrate_scaled refuses for the shared
 * arguments (a pitch that is no multiple of 4 or shorter than a row, planes outside the volume); an empty or reversed plane range; an axis
 * outside 1 .. 262140; max_weight outside [1, 1 << 24]; voxel_size or tranc_dist not positive and finite. */
#define XS_REINTEGRATE_MAX_OPS 8
#define XS_REINTEGRATE_NO_CULL 1u
typedef struct xs_reintegrate_op {
    int sign;                   /* -1: take the observation out, +1: put it in */
    const float *depth_scaled;  /* device, rows x cols, the image xs_scale_depth gives; ops may share one */
    float Rv2c18[18], tv2c6[6]; /* the complex pose, as xs_integrate_scaled takes it */
} xs_reintegrate_op;
int xs_tsdf_reintegrate(int ops, const xs_reintegrate_op *ops_host, size_t scaled_step, int rows, int cols, const float *intr4,
                        int max_weight, const int *res, float voxel_size, float tranc_dist, float threshold,
                        float *value, int *weight, float *grad, size_t vol_step, int z0, int z1,
                        unsigned long long *counts4_dev, unsigned flags, void *stream);

/* ---- what differs between the volume and a second volume, as two masks (xs_diff.hip) ---------------------------
 * No counterpart in the reference.  THIS map is (value, weight, step, res), the OTHER map (src_*); layouts, pitches and xform12 are those of
 * the merge above, the pointers at plane 0, the whole volume always.  Neither volume is modified.  `only_this_mask` and `only_other_mask`:
 * two different buffers of the frontier mask's size for res (8 bytes per brick of THIS map, 8-byte aligned device memory), in that
 * mask's layout: one 64-bit word per brick of 4 x 4 x 4 voxels, brick (bx, by, bz) at (bz BY + by) BX + bx, voxel (lx, ly, lz) at bit
 * lx + 4 ly + 16 lz, overhang bits clear: the frontier's label and cluster calls take them as they are.  The call writes EVERY word of both
 * masks, the caller need not clear them.  counts3_dev (device): {compared, only_this, only_other} are INCREMENTED by the numbers of such
 * voxels, with integer atomics, one add per counter and workgroup.  `workspace`: the diff's workspace size for (res, src_res) in bytes of
 * device memory (may be NULL with XS_DIFF_NO_CULL).  No synchronisation.
 *
 * Destination voxel (x, y, z) of THIS map, every operation float32 in the order written:
 *   1. The source sample: steps 1 to 3 of the merge, word for word: g_a; the voxel passes only with 0 <= g_a <= float(S_a - 1) on every axis;
 *      b_a = floor(g_a), f_a = g_a - float(b_a); only the needed corners are read; ws = the smallest weight of the needed corners.
 *   2. The other map is OBSERVED here iff the voxel passed the merge's step 2 and ws >= min_weight (ws is not clamped: there is no
 *      max_weight).  This map is OBSERVED here iff its own weight wp >= min_weight.  The voxel is COMPARED iff both are observed.
 *   3. For a compared voxel s is the merge's step 4 on the value array alone (there is no grad argument): along x, then y, then z, a stage
 *      being lo * (1.0f - f_a) + hi * f_a and its lower operand itself on an axis with f_a == 0 (-0 stays -0).  v = this map's value.
 *   4. only_this iff v < lo && s >= hi (matter here, firmly free there); only_other iff s < lo && v >= hi.  With lo <= hi the two exclude
 *      each other.  (The layers above default to lo = 0, hi = 0.5: OCCUPIED in the observation grid is value < 0, and free space the
 *      integrate step has seen holds 1.  The comparison with lo is strict, so -0.0f is not below lo = 0, as in that grid.)
 *   5. The voxel's bit of each mask is its class; the bit of a voxel that is not compared is clear in both.
 *   6. The counts: the number of compared voxels, and of the set bits of each mask.
 * The cull is the merge's (a tile of 64 x 4 x 16 destination voxels whose source index box misses the source, or touches only bricks of
 * 4 x 4 x 4 source voxels with no weight >= min_weight, stores zero words and leaves) and changes no bit; XS_DIFF_NO_CULL switches it off.
 * A voxel with wp < min_weight reads nothing of the source.  No output depends on scheduling.
 * hipErrorInvalidValue, with nothing launched and nothing written: what the merge refuses for these arguments (a null array, resolution
 * or xform12, or workspace unless XS_DIFF_NO_CULL; an axis outside 1 .. 262140; a pitch that is no multiple of 4 or shorter than a row;
 * min_weight < 1; an entry of xform12 that is not finite; a source array equal to its counterpart of this map); lo or hi not finite, or
 * lo > hi; a null mask or counts pointer; the two masks equal, or one not 8-byte aligned; a `res` that has no frontier mask (the masks must
 * be labelable): for it the workspace size is 0 too. */
#define XS_DIFF_NO_CULL 1u
size_t xs_tsdf_diff_workspace_bytes(const int *res, const int *src_res);
int xs_tsdf_diff(const float *value, const int *weight, size_t step, const int *res, const float *src_value, const int *src_weight, size_t src_step,
                 const int *src_res, const float *xform12, int min_weight, float lo, float hi, unsigned flags, void *only_this_mask,
                 void *only_other_mask, unsigned long long *counts3_dev, void *workspace, void *stream);

/* ---- the volume as bricks of 8 x 8 x 8 voxels, one word or 512 per array (xs_pack.hip) ---------------------------
 * No counterpart in the reference.  The kernels behind the brick-sparse checkpoint XSTSDF3 ("Checkpoint formats").  The arrays
 * are given at the FIRST STORED PLANE, in the layout of every call here (row Y * z + y, x contiguous) with one pitch `step` (bytes) shared by the
 * three; `planes` is the number of stored planes (res[2] for a whole volume), res[2] itself is only range-checked.  Byte offsets row * step are
 * computed in 64 bits.  None of the calls synchronises.
 *
 * Bricks: nbx, nby, nbz = ceil(res[0] / 8), ceil(res[1] / 8), ceil(planes / 8); brick (bx, by, bz) has index (bz nby + by) nbx + bx and holds
 * voxels 8 b + (i, j, k), i, j, k in 0 .. 7, those inside X x Y x planes being its in-volume voxels; (8 bx, 8 by, 8 bz), its first voxel, always
 * is.  All comparisons are on 32-bit WORDS, never on floats: +0.0 differs from -0.0, two NaNs with different payloads differ, one NaN pattern
 * equals itself.
 *   class:   bit 0 (value), bit 1 (weight), bit 2 (grad): set iff some in-volume word of that array differs from the array's word at the
 *            brick's first voxel (the array is DENSE in the brick); clear: the array is UNIFORM there.
 *   words:   a uniform array takes 1 word of the payload (the first voxel's), a dense array 512: the word of local voxel (i, j, k) at
 *            i + 8 j + 64 k, positions outside the volume holding the first voxel's word.  Within a brick: value, weight, grad.
 *   offsets: offsets[b] = the sum of the words of bricks 0 .. b - 1 (uint64), offsets[nbricks] the payload's length in words.
 * So class bytes, offsets and payload are a pure function of the volume's bits, and no output depends on scheduling (the sums are integer).
 *
 * The brick count for (res, planes), 0 where the calls below would refuse them; and the workspace of classify and of the offsets call, in bytes
 * of device memory (0 likewise). */
size_t xs_tsdf_pack_bricks(const int *res, int planes);
size_t xs_tsdf_pack_workspace_bytes(const int *res, int planes);
/* Fills cls_dev[nbricks] (each byte written once, no atomics) and offsets_dev[nbricks + 1] from the volume, which is only read. */
int xs_tsdf_pack_classify(const float *value, const int *weight, const float *grad, size_t step, const int *res, int planes,
                          unsigned char *cls_dev, unsigned long long *offsets_dev, void *workspace, void *stream);
/* The offsets alone, from class bytes that came from elsewhere (a file): bits 3 .. 7 of a class byte are ignored here, a reader validates them
 * beforehand.  workspace: the workspace size of any (res, planes) with this brick count.  Refuses a null pointer and nbricks outside [1, 2^31). */
int xs_tsdf_pack_offsets(const unsigned char *cls_dev, size_t nbricks, unsigned long long *offsets_dev, void *workspace, void *stream);
/* Writes the payload words of bricks [brick0, brick1) to payload_dev[0 .. offsets[brick1] - offsets[brick0]): the volume is only read.  The range
 * exists so that a host can stream a volume of any size through a buffer of fixed size: a brick takes at most 1536 words. */
int xs_tsdf_pack_gather(const float *value, const int *weight, const float *grad, size_t step, const int *res, int planes,
                        const unsigned char *cls_dev, const unsigned long long *offsets_dev, size_t brick0, size_t brick1, unsigned *payload_dev,
                        void *stream);
/* The inverse: writes every in-volume voxel of bricks [brick0, brick1) from payload_dev (laid out as the gather of the same range leaves it) and
 * nothing else: no pitch padding, no row outside those bricks.
 * hipErrorInvalidValue, with nothing launched, from classify, gather and unpack alike: a null pointer; res[0], res[1], res[2] or planes outside
 * 1 .. 262140, res[1] * planes of 2^31 and more, or 2^31 bricks and more; a pitch that is no multiple of 4 or shorter than a row; an empty or
 * reversed brick range or one outside [0, nbricks]. */
int xs_tsdf_unpack(float *value, int *weight, float *grad, size_t step, const int *res, int planes, const unsigned char *cls_dev,
                   const unsigned long long *offsets_dev, size_t brick0, size_t brick1, const unsigned *payload_dev, void *stream);

/* ---- aligning a second volume to the volume: Gauss-Newton terms over the band (xs_align.hip) -------------------
 * No counterpart in the reference.  The residual of a band voxel of THIS map is "the other map, resampled at the voxel under a complex-seeded
 * affine index map, minus this map": the sample xs_tsdf_merge would average in, at the position it would use.  `index`: the band index of THIS
 * map (xs_tsdf_band_build); only its keys, values and count are used.  The source: value and weight arrays of the other map at plane 0, one
 * pitch, the layout of xs_tsdf_merge; it is only read.  maps144xN: host array, per transform six seeded maps (the generators of the rigid
 * transform, x-slam_amd/host/align_host.hpp: xs_host_align_seeded_maps) of 12 complex entries (re, im) in xform12's order.  Transform n's 29
 * sums land at out29xN_dev + 29 n, in the layout of xs_tsdf_gauss_newton_terms.
 *
 * Index entry (x, y, z, gt), transform n; m_k = seed k's map, complex float32 in the arithmetic of csrc/xs_complex.h, every operation in the
 * order written (the library is built with -ffp-contract=off):
 *   1. g_a = ((m_k[3a] * float(x) + m_k[3a + 1] * float(y)) + m_k[3a + 2] * float(z)) + m_k[9 + a]  (complex times real, complex sums).  With
 *      the maps of xs_host_align_seeded_maps Re g_a is merge_index's value, bit for bit, for every seed.
 *   2. The cell comes from seed 0: the entry is dropped unless 0 <= Re g_a < float(S_a - 1) on every axis (S: the source resolution; a NaN
 *      fails).  b_a = floor(Re g_a); for every seed f_a = g_a - float(b_a) (complex) and c_a = 1.0f - f_a.  All eight corners b + {0, 1}^3
 *      are read on every entry that gets this far (the derivative needs the neighbours even where Re f_a = 0); no other source voxel is.
 *   3. The entry is dropped unless all eight corner weights are >= min_weight; a dropped entry loads no value.
 *   4. F: along x the real corner values, lo * c_0 + hi * f_0 (real times complex); then along y and along z, lo * c_a + hi * f_a (complex
 *      times complex).
 *   5. r_k = F - gt.  The entry is dropped if |Re r_k| > max_residual for any seed.
 *   6. A kept entry adds, in double: Im r_j * Im r_k (j <= k, row-major) to [0, 21), Im r_k * Re r_0 to [21, 27), (Re r_0)^2 to [27], 1 to [28].
 * Order: the entries are dealt out in chunks of 64 as for xs_tsdf_pose_hessian_band and folded in a fixed order that is a function of
 * index->count alone: two launches on the same inputs give the same bits, and transform n's sums do not depend on `transforms`, on n or on
 * the other transforms.  No floating-point atomics.  An index with count 0 yields zeros.
 * Workspace: xs_tsdf_align_workspace_bytes(transforms) bytes (0 for transforms outside 1 .. XS_ALIGN_MAX_TRANSFORMS): one arrival ticket per
 * transform in its first 256 bytes, the maps, the records.  Zero the first 256 bytes ONCE after allocation (xs_tsdf_reduce_workspace_init);
 * every launch leaves them zero.  One launch at a time per workspace.  No synchronisation.
 * hipErrorInvalidValue, with nothing launched: transforms outside 1 .. 32; a null pointer; an index that was not built (the checks of
 * xs_tsdf_pose_hessian_band); a source axis outside 2 .. 262140, or rows (S_1 S_2) that do not fit an int; a pitch that is no multiple of 4
 * or shorter than a row; min_weight < 1; max_residual not finite or <= 0; a map entry that is not finite. */
#define XS_ALIGN_MAX_TRANSFORMS 32
size_t xs_tsdf_align_workspace_bytes(int transforms);
int xs_tsdf_align_terms(int transforms, const xs_band_index *index, const float *src_value, const int *src_weight, size_t src_step,
                        const int *src_res, const float *maps144xN, int min_weight, float max_residual, void *workspace, double *out29xN_dev,
                        void *stream);

/* ---- the loss of many map-to-map transforms in one pass over the band (xs_align.hip) ---------------------------
 * No counterpart in the reference.  The loss and voxel count of "the other map resampled under m minus this map" over the band index of THIS
 * map, for `transforms` (1 .. XS_ALIGN_SCORE_MAX_TRANSFORMS) real index maps in one launch: what xs_tsdf_score_poses_band is to a depth frame.
 * Real-valued: no seeds, no derivative.  The index, the source and its layout: as for xs_tsdf_align_terms.  xform12xP: host array, transform
 * p's xform12 (xs_host_merge_affine) at + 12 p.  Transform p's two doubles land at out2xP_dev + 2 p: {sum r^2, count}.
 *
 * Scored entries: index entries e = stride i, i = 0 .. ceil(count / stride) - 1 (stride 1: the whole band); scored entry i belongs to chunk
 * i / 64, lane i % 64.  Scored entry (x, y, z, gt), transform p, m = xform12xP + 12 p; every operation float32 in the order written (the
 * library is built with -ffp-contract=off):
 *   1. g_a = ((m[3a] * float(x) + m[3a + 1] * float(y)) + m[3a + 2] * float(z)) + m[9 + a]: xs_tsdf_merge's step 1, and with
 *      m = xs_host_merge_affine(T) the real part of xs_tsdf_align_terms' g_a, bit for bit.
 *   2. The entry is dropped unless 0 <= g_a < float(S_a - 1) on every axis (xs_tsdf_align_terms' cell rule; a NaN fails).  b_a = floor(g_a),
 *      f_a = g_a - float(b_a), c_a = 1.0f - f_a.
 *   3. The entry is dropped, without loading a value, unless all eight corner weights b + {0, 1}^3 are >= min_weight.
 *   4. F: along x, then y, then z, each stage lo * c_a + hi * f_a (done even where f_a == 0).
 *   5. r = F - gt.  The entry is kept only if |r| <= max_residual (a NaN drops).
 *   6. A kept entry adds the float32 product r * r and counts 1.
 * Order (xs_tsdf_score_poses_band's): per (chunk, transform) a six-level pairwise float tree across the wave over kept-or-zero terms,
 * everything after that in double, in an order that is a function of index->count and stride alone: two launches on the same inputs give
 * the same bits, and transform p's two numbers do not depend on `transforms`, on p or on the other transforms.  All terms are >= 0, so
 * |sum - sum of the float32 terms in double| <= 8 * 2^-24 * sum.  No floating-point atomics.  An index with count 0 yields zeros.
 * Workspace: xs_tsdf_score_transforms_workspace_bytes(transforms) bytes (0 outside 1 .. XS_ALIGN_SCORE_MAX_TRANSFORMS): one arrival ticket per
 * tile of 64 transforms in its first 256 bytes, the maps, the records.  Zero the first 256 bytes ONCE after allocation
 * (xs_tsdf_reduce_workspace_init); every launch leaves each ticket at zero again.  One launch at a time per workspace.  No synchronisation.
 * hipErrorInvalidValue, with nothing launched: xs_tsdf_align_terms' refusals, transforms outside 1 .. 4096, stride < 1. */
#define XS_ALIGN_SCORE_MAX_TRANSFORMS 4096
size_t xs_tsdf_score_transforms_workspace_bytes(int transforms);
int xs_tsdf_score_transforms(int transforms, const xs_band_index *index, int stride, const float *src_value, const int *src_weight,
                             size_t src_step, const int *src_res, const float *xform12xP, int min_weight, float max_residual, void *workspace,
                             double *out2xP_dev, void *stream);

/* ---- depth, normal and shaded views of a map, many views in one launch (xs_render.hip) ------------------------
 * No counterpart in the reference, whose only ray caster is the tracker's (xs_raycast above: complex arithmetic, normalised rays, one
 * view, the tracking buffers).  This one is real arithmetic at any intrinsics and image size, and its depth is measured along the camera's
 * z: the image is what a depth sensor at that pose would report.  The volume (value, weight, one pitch vol_step in bytes, rows in
 * (z * Y + y) order, the pointers at plane 0) is only read; byte offsets row * vol_step are computed in 64 bits.
 *
 * xs_render_workspace_bytes: the workspace for `res` in bytes of device memory (256-byte aligned): a header, the staging area of one
 * launch's poses, and the BRICK MASK, one bit per brick of 8 x 8 x 8 voxels.  0 for a null or unusable resolution.  Host only.
 * xs_render_mask_build: bit bx & 31 of word (bz BY + by) WX + (bx >> 5), with BX, BY, BZ = ceil(res / 8) and WX = ceil(BX / 32), is set iff
 * brick (bx, by, bz) holds a voxel with value < 0 && weight >= min_weight (min_weight below 1 means 1); the other bits of a row's last
 * word are clear.  One read of the two arrays, one writer per word, no atomics.  The call then records (res, min_weight) in the header.  The
 * mask describes the volume as it was when the call ran: rebuild it after the volume changes.  No synchronisation.
 *
 * xs_render_views: `views` (1 .. XS_RENDER_MAX_VIEWS) real camera-to-volume poses, host arrays Rc2v9xP + 9 p (row-major) / tc2v3xP + 3 p,
 * copied into the workspace's staging area (one launch at a time per workspace), each rendering a rows x cols image (1 .. 4096 each) of a
 * camera with intrinsics intr4 = {fx, fy, cx, cy}, all in one launch.  Every float operation below is one IEEE float32 operation in the
 * order written (the library is built -ffp-contract=off; divides and square roots correctly rounded), there are no floating-point
 * atomics: a float32 model on the host reproduces every output bit, two launches give the same bits, and view p's output does not
 * depend on `views`, on p or on the other views.  opts (NULL: all defaults): t_near, t_far = 0, 0 means 0.2, 5.0; step = 0 means
 * voxel_size; min_weight below 1 means 1; shade_mode 0 (headlight) is the only mode.
 *   pixel (x, y):  dx = (float(x) - cx) / fx,  dy = (float(y) - cy) / fy,  d[c] = (R[c][0] * dx + R[c][1] * dy) + R[c][2]  (not normalised:
 *                  t is depth along the camera's z; the unprojection xs_create_vmap applies to a depth image)
 *   sample k = 0 .. n - 1:  t_k = t_near + float(k) * step (no running sum), n = the number of k with t_k < t_far;  p[c] = tc2v[c] + t_k * d[c];
 *                  q[c] = p[c] / voxel_size; the voxel is floor(q[c]) and lies inside iff 0 <= q[c] < float(res[c]) on every axis (a NaN
 *                  is outside).  The sample's state s_k is NONE where the voxel is outside or its weight < min_weight, otherwise its value.
 *   march, k = 0 .. n - 2, the first k at which s_k and s_k+1 are both values and
 *                  s_k < 0 && s_k+1 > 0:  the ray ends as BACKFACE;
 *                  s_k > 0 && s_k+1 < 0:  the ray is REFINED and ends, as HIT or as REJECTED.
 *                  A NONE sample, and a value of 0.0f or -0.0f, never ends a ray.  A ray nothing ends is NONE.
 *   F(P), the trilinear value at a point P (metres):  g[c] = P[c] / voxel_size - 0.5f; REFUSED unless 0 <= g[c] <= float(res[c] - 1) on
 *                  every axis; b[c] = floor(g[c]), f[c] = g[c] - float(b[c]); only the corners b + e with e[c] = 1 on axes with f[c] > 0
 *                  are read; REFUSED if the smallest weight among them < min_weight; the values are interpolated along x, then y, then
 *                  z, a stage being lo * (1.0f - f[c]) + hi * f[c], and its lower operand itself on an axis with f[c] == 0 (the
 *                  sampling rule of xs_tsdf_merge, steps 2 to 4, on the value array).
 *   refinement:    F0 = F(p(t_k)), F1 = F(p(t_k+1)), with p(t)[c] = tc2v[c] + t * d[c].  REJECTED if F0 or F1 is refused, or
 *                  !(F0 >= 0 && F1 <= 0), or F1 - F0 == 0.  Otherwise HIT with ts = t_k - step * (F0 / (F1 - F0)).
 * Outputs, each optional (NULL: not wanted; another output's bits do not depend on it), dense and view-major:
 *   depth_f32 [P][rows][cols]     ts; 0.0f where the ray is no HIT.
 *   depth_u16 [P][rows][cols]     r = rint(ts * 1000.0f) where 1 <= r <= 65535, else 0: millimetres, as xs_scale_depth takes them.
 *   normal    [P][3][rows][cols]  in the volume frame, pointing into free space:  Q = p(ts), h = 0.5f * voxel_size,
 *                                 G[c] = F(Q + h e_c) - F(Q - h e_c) (only coordinate c changes), gg = (G[0] * G[0] + G[1] * G[1]) + G[2] * G[2],
 *                                 N[c] = G[c] / sqrt(gg).  The NaN 0x7fffffff in all three where the ray is no HIT, one of the six
 *                                 samples is refused, or !(gg > 0).
 *   shade     [P][rows][cols]     uint8, headlight:  nd = (N[0] * d[0] + N[1] * d[1]) + N[2] * d[2],  dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2],
 *                                 rint(255.0f * min(1.0f, |nd| / sqrt(dd))); 0 where the ray is no HIT or has no normal.
 *   counts4xP [P][4]              uint32 {hit, backface, rejected, none} of the view's rows * cols rays; zeroed by the call on the
 *                                 stream, then integer atomics, one per counter and workgroup.
 * The cull (opts->cull != 0): a sample whose brick's mask bit is clear cannot be the negative side of either event, so it is read only
 * when its neighbour sample turns out to be a negative value.  It changes no bit of any output.  It needs a mask built in this workspace
 * for this res with a min_weight not above the call's: the call reads the header back on the stream and waits for it (the one
 * synchronisation; without the cull there is none).
 * hipErrorInvalidValue, with nothing launched and every output untouched: views outside 1 .. XS_RENDER_MAX_VIEWS; rows or cols outside
 * 1 .. 4096; a null pose, intrinsics, resolution, volume or workspace pointer; every output null; a pose or intrinsic entry that is not
 * finite; fx or fy equal to 0; voxel_size not positive and finite; a pitch that is no multiple of 4 or shorter than a row; step < 0 or
 * not finite; a range that is not finite or has t_far <= t_near; more than 4096 samples; an axis outside 1 .. 262140 or rows that do not
 * fit an int (the merge's rule); opts->struct_bytes not sizeof(xs_render_opts); a shade_mode other than 0; the cull without such a mask. */
#define XS_RENDER_MAX_VIEWS 64
typedef struct xs_render_opts {
    unsigned struct_bytes;     /* sizeof(xs_render_opts) */
    float t_near, t_far;       /* depth range along the camera's z; 0, 0 = 0.2, 5.0 */
    float step;                /* depth increment per sample; 0 = voxel_size */
    int min_weight;            /* a voxel with a smaller weight is unseen; below 1 = 1 */
    int cull;                  /* not 0: consult the workspace's brick mask */
    int shade_mode;            /* 0: headlight */
} xs_render_opts;
size_t xs_render_workspace_bytes(const int *res);
int xs_render_mask_build(const float *value, const int *weight, size_t vol_step, const int *res, int min_weight, void *workspace, void *stream);
int xs_render_views(int views, const float *Rc2v9xP, const float *tc2v3xP, const float *intr4, int rows, int cols, const float *value,
                    const int *weight, size_t vol_step, const int *res, float voxel_size, const xs_render_opts *opts, void *workspace,
                    float *depth_f32, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4xP, void *stream);

/* ---- the map sampled at the caller's points, and at a depth frame's pixels (xs_sample.hip) ---------------------
 * No counterpart in the reference.  What is the signed distance here, which way does it grow, has this place been seen: F(P) of
 * xs_render_views above (the same device function, xs_trilinear.h) applied to points the caller supplies, one lane per point, all in one
 * launch.  The volume is given as xs_render_views takes it, plus an optional `grad` array with the same pitch; it is only read; byte
 * offsets row * vol_step are computed in 64 bits.  Every float operation below is one IEEE float32 operation in the order written (the
 * library is built -ffp-contract=off), there are no floating-point atomics, no synchronisation and no workspace: a float32 model on the
 * host reproduces every output bit, two launches give equal bytes, and point i's outputs depend on nothing but point i, the volume and
 * the options (not on n, not on i).  opts (NULL: all defaults): min_weight below 1 means 1.
 *
 * xs_tsdf_sample_points: n points (1 .. 2^30), a device array points3xN_dev + 3 i of float32 metres (4-byte aligned).  xform12 (host,
 * optional): row-major R, then t.
 *   with a transform:  P[c] = ((R[c][0] * p[0] + R[c][1] * p[1]) + R[c][2] * p[2]) + t[c];   without one:  P = p, the point's bits as they are.
 * xs_tsdf_sample_depth: the points of a depth image's pixels: u16 millimetres, pitched (depth_step bytes per row), rows x cols (1 .. 4096
 * each), a camera with intrinsics intr4 = {fx, fy, cx, cy} at the real camera-to-volume pose Rc2v9 (row-major), tc2v3 (host arrays).
 *   pixel (x, y), D = depth[y][x]:  NO_DEPTH if D < 200 || D > 5000 (xs_scale_depth's rule); otherwise z = float(D) / 1000.f,
 *                  dx = (float(x) - cx) / fx,  dy = (float(y) - cy) / fy,  d[c] = (R[c][0] * dx + R[c][1] * dy) + R[c][2],
 *                  P[c] = tc2v[c] + z * d[c]:  xs_render_views' p(t) at t = z.
 * Outputs, each optional (NULL: not wanted; another output's bits do not depend on it); per point [N] / [N][3], per pixel dense
 * [rows][cols] / [3][rows][cols]:
 *   status    uint8    0 OUTSIDE: F(P) refused by its range test (a NaN or an infinite coordinate is outside);  1 UNSEEN: refused because the
 *                      smallest weight among the needed corners < min_weight;  2 OK;  3 NO_DEPTH (the depth call only).
 *   value     float32  F(P) exactly as xs_render_views defines it: voxel centres at (i + 0.5) voxel_size, only the corners on axes with
 *                      f > 0 read.  The NaN 0x7fffffff where the status is not OK.  In units of the truncation distance, like the volume.
 *   dvalue    float32  the same interpolation (the same corners, fractions and order) applied to the grad array; 0x7fffffff where not OK.
 *   gradient  float32  G[c] / voxel_size,  G[c] = F(P + h e_c) - F(P - h e_c) (only coordinate c changes),  h = 0.5f * voxel_size:
 *                      xs_render_views' G, in value per metre.  It is the derivative of the continuous interpolant averaged over one
 *                      voxel, continuous across cell faces; its direction is the render's normal.  0x7fffffff in all three where the
 *                      centre is not OK or any of the six samples is refused.
 *   counts4   unsigned long long [4] = {outside, unseen, ok, no_depth}; zeroed by the call on the stream, then integer atomics, one per
 *                      counter and workgroup.
 * hipErrorInvalidValue, with nothing launched and every output untouched: n outside 1 .. 2^30; rows or cols outside 1 .. 4096; a null
 * points, depth, pose, intrinsics, resolution or volume pointer; every output null; dvalue wanted without grad; an output pointer equal to
 * the points (depth) pointer; a transform, pose or intrinsic entry that is not finite; fx or fy equal to 0; voxel_size not positive and
 * finite; xs_render_views' pitch and resolution rules; opts->struct_bytes not sizeof(xs_sample_opts); a depth pitch shorter than a row or
 * odd. */
typedef struct xs_sample_opts {
    unsigned struct_bytes;     /* sizeof(xs_sample_opts) */
    int min_weight;            /* a voxel with a smaller weight is unseen; below 1 = 1 */
} xs_sample_opts;
int xs_tsdf_sample_points(long long n, const float *points3xN_dev, const float *xform12, const float *value, const int *weight, const float *grad,
                          size_t vol_step, const int *res, float voxel_size, const xs_sample_opts *opts, unsigned char *status, float *value_out,
                          float *dvalue, float *gradient3xN, unsigned long long *counts4, void *stream);
int xs_tsdf_sample_depth(const uint16_t *depth_dev, size_t depth_step, int rows, int cols, const float *intr4, const float *Rc2v9, const float *tc2v3,
                         const float *value, const int *weight, const float *grad, size_t vol_step, const int *res, float voxel_size,
                         const xs_sample_opts *opts, unsigned char *status, float *value_out, float *dvalue, float *gradient3,
                         unsigned long long *counts4, void *stream);

/* ---- registering a point cloud to the volume: Gauss-Newton terms over the points (xs_register.hip) ---------------
 * No counterpart in the reference.  The residual of a point p under a rigid transform is the map's value at the transformed point, its
 * Jacobian the map's gradient there: the 29 sums of the normal equations for `transforms` (1 .. XS_REGISTER_MAX_TRANSFORMS) transforms over
 * the same n points (1 .. 2^30) in one launch.  points3xN_dev: xs_tsdf_sample_points' device array.  xform12xN: host array, never null,
 * transform m's row-major R, then t at + 12 m; it is copied into the launch's arguments and may be reused when the call returns.  The volume
 * (value, weight, one pitch vol_step in bytes, rows in (z * Y + y) order, the pointers at plane 0) is only read; byte offsets row * vol_step
 * are computed in 64 bits.  Transform m's 29 doubles land at out29xN_dev + 29 m, in the layout of xs_tsdf_gauss_newton_terms; nothing else
 * but the workspace is written.
 *
 * Transform m, point p; every float operation is one IEEE float32 operation in the order written (the library is built -ffp-contract=off):
 *   1. P[c] = ((R[c][0] * p[0] + R[c][1] * p[1]) + R[c][2] * p[2]) + t[c]:  xs_tsdf_sample_points' transformed point.
 *   2. (status, r, g[3]) = the status, value and gradient xs_tsdf_sample_points defines at P with this min_weight and no grad array: the bytes
 *      that call would write for the point.
 *   3. The point is DROPPED if its status is not OK;  or the gradient is refused (one of the six samples at +- half a voxel is not OK: the
 *      three gradient words are the NaN 0x7fffffff);  or fabsf(r) > max_residual.
 *   4. J[0] = g[0], J[1] = g[1], J[2] = g[2];  J[3] = P[1] * g[2] - P[2] * g[1];  J[4] = P[2] * g[0] - P[0] * g[2];
 *      J[5] = P[0] * g[1] - P[1] * g[0]  (two products and one subtraction each):  the derivative of F(exp(delta) T p) at delta = 0 for
 *      delta = (translation, rotation), the order of se3Exp and of xs_host_align_step.
 *   5. A kept point adds, in double: double(J[j]) * double(J[k]) (j <= k, row-major) to [0, 21), double(J[k]) * double(r) to [21, 27),
 *      double(r) * double(r) to [27], 1 to [28].  Every product of two float32 factors is exact in double.
 * No seed and no step h: the sums are the normal equations as they stand (xs_host_align_step takes them unscaled).
 * Order (xs_tsdf_align_terms' with "band entry" read as "point"): point i belongs to chunk i / 64, lane i % 64; wave w of workgroup (b, m)
 * takes chunks 4 b + w, + 4 nblocks, ... with nblocks = clamp(ceil(ceil(n / 64) / 4), 1, 4096), and adds its points' terms to 29 double sums
 * per lane in that order; the lanes, the four waves and the workgroups' records are then added in a fixed order with one arrival ticket per
 * transform.  The order is a function of n alone: two launches on the same inputs give equal bytes, and transform m's 29 doubles depend on
 * nothing but m's twelve floats, the points and the volume — not on m, on `transforms` or on the other transforms.  No floating-point
 * atomics.  A transform that keeps no point yields 29 zeros.
 * Workspace: xs_tsdf_register_workspace_bytes(transforms) bytes (0 for transforms outside 1 .. XS_REGISTER_MAX_TRANSFORMS): one arrival ticket
 * per transform in its first 256 bytes, then the records.  Zero the first 256 bytes ONCE after allocation (xs_tsdf_reduce_workspace_init);
 * every launch leaves them zero.  One launch at a time per workspace.  No synchronisation.
 * hipErrorInvalidValue, with nothing launched and nothing written: transforms outside 1 .. 32; n outside 1 .. 2^30; a null points,
 * transforms, value, weight, resolution, workspace or output pointer; xs_tsdf_sample_points' resolution, pitch and voxel-size rules;
 * min_weight < 1; max_residual not finite or <= 0; a transform entry that is not finite. */
#define XS_REGISTER_MAX_TRANSFORMS 32
size_t xs_tsdf_register_workspace_bytes(int transforms);
int xs_tsdf_register_terms(int transforms, long long n, const float *points3xN_dev, const float *xform12xN, const float *value, const int *weight,
                           size_t vol_step, const int *res, float voxel_size, int min_weight, float max_residual, void *workspace,
                           double *out29xN_dev, void *stream);

/* ---- the loss of many transforms of a point cloud in one pass over the points (xs_register.hip: k_register_score) --
 * No counterpart in the reference.  {sum r^2, count} of the residual above, without its Jacobian, for `transforms` (1 ..
 * XS_REGISTER_SCORE_MAX_TRANSFORMS) transforms over every stride-th of the n points in one launch: what xs_tsdf_score_transforms is to a
 * second map, and what finds the transform xs_tsdf_register_terms starts from when nobody supplies one.  The points, the volume and the
 * 64-bit row offsets: as for xs_tsdf_register_terms.  xform12xP: host array, never null, transform p's row-major R, then t at + 12 p; the call
 * copies it into the workspace on the stream (hipMemcpyAsync from pageable memory: it may be reused when the call returns).  Transform p's
 * two doubles land at out2xP_dev + 2 p: {sum r^2, count}; nothing but the pairs and the workspace is written.
 *
 * Scored points: points stride i, i = 0 .. ceil(n / stride) - 1 (stride 1: the whole cloud); scored point i belongs to chunk i / 64, lane
 * i % 64.  Scored point q, transform p; every float operation is one IEEE float32 operation in the order written:
 *   1. P[c] = ((R[c][0] * q[0] + R[c][1] * q[1]) + R[c][2] * q[2]) + t[c]:  xs_tsdf_sample_points' transformed point.
 *   2. (status, r) = the status and value xs_tsdf_sample_points defines at P with this min_weight and no grad array (the same device
 *      function, F of xs_trilinear.h: g = P / voxel_size - 0.5f, only the corners on axes with a fraction > 0 read and tested).
 *   3. The point is KEPT iff status == OK && fabsf(r) <= max_residual (a NaN drops).  There is no gradient and no gradient gate: a point
 *      whose gradient xs_tsdf_register_terms refuses (one of its six outer samples is not OK) counts here, so a transform's count may exceed
 *      that call's, never fall below it.
 *   4. A kept point adds the float32 product r * r and counts 1.
 * Order (xs_tsdf_score_transforms'): wave w of workgroup (b, tile) takes chunks 4 b + w, + 4 nblocks, ... with nblocks =
 * clamp(ceil(ceil(scored / 64) / 4), 1, 1024); per (chunk, transform) a six-level pairwise float tree across the wave over kept-or-zero
 * terms, everything after that in double: a lane per transform adds its chunks' tree sums in order, then the four waves in wave order, one
 * record per workgroup, one arrival ticket per tile of 64 transforms, and the tile's last workgroup adds the records in index order.  The
 * order is a function of ceil(n / stride) alone: two launches on the same inputs give equal bytes, and transform p's pair does not depend on
 * `transforms`, on p or on the other transforms.  All terms are >= 0, so |sum - sum of the float32 terms in double| <= 8 * 2^-24 * sum.  No
 * floating-point atomics.  A transform that keeps no point yields {+0.0, 0}.
 * Workspace: xs_tsdf_score_points_workspace_bytes(transforms) bytes (0 outside 1 .. XS_REGISTER_SCORE_MAX_TRANSFORMS): one arrival ticket per
 * tile in its first 256 bytes, the transforms, the records.  Zero the first 256 bytes ONCE after allocation (xs_tsdf_reduce_workspace_init);
 * every launch leaves each ticket at zero again.  One launch at a time per workspace.  No synchronisation.
 * hipErrorInvalidValue, with nothing launched and nothing written: xs_tsdf_register_terms' refusals, transforms outside 1 .. 4096,
 * stride < 1. */
#define XS_REGISTER_SCORE_MAX_TRANSFORMS 4096
size_t xs_tsdf_score_points_workspace_bytes(int transforms);
int xs_tsdf_score_points(int transforms, long long n, int stride, const float *points3xN_dev, const float *xform12xP, const float *value,
                         const int *weight, size_t vol_step, const int *res, float voxel_size, int min_weight, float max_residual, void *workspace,
                         double *out2xP_dev, void *stream);

/* ---- fusing a point cloud into the volume: a scatter of integers, then a fold (xs_fuse.hip) ---------------------
 * No counterpart in the reference.  Every other call that writes the volume takes a depth image or a second volume and gathers; this one
 * takes points with a sensor origin, walks each point's ray, and SCATTERS: one lane per point, adding to voxels that other lanes add to as
 * well.  What is added is an integer, so the order of the additions cannot matter: xs_tsdf_fuse_points_accumulate adds, per ray and voxel, a
 * fixed-point observation and a count to one 64-bit word of an accumulator with one integer atomic whose result is not used, and
 * xs_tsdf_fuse_points_fold turns the accumulator into one weighted observation per touched voxel, averaged into the volume by the merge's
 * rule, and leaves the accumulator zero.  No floating-point atomics: two runs, or the same points in any order, give equal bytes, and a
 * host model adding uint64 words reproduces every word.  Every float operation below is one IEEE float32 operation in the order written (the
 * library is built -ffp-contract=off).  No synchronisation.
 *
 * The accumulator: xs_tsdf_fuse_accumulator_bytes(res) bytes (8 X Y Z; 0 for a null or unusable resolution), dense, the word of voxel
 * (x, y, z) at index (z Y + y) X + x computed in 64 bits; count in bits 40 .. 63, the sum of q in bits 0 .. 39.  Zero it ONCE after
 * allocation; the fold leaves every word of its planes zero.  Several accumulates may precede one fold, as long as no more than
 * XS_FUSE_MAX_POINTS (2^24 - 1) points lie between two folds: q <= 2^16, so neither field can overflow.
 *
 * xs_tsdf_fuse_points_accumulate: n points (1 .. XS_FUSE_MAX_POINTS), xs_tsdf_sample_points' device array; xform12 (host, optional): row-major
 * R, then t; origin3 (host): the sensor origin in the points' frame; opts: never null.  Point p:
 *   1. With a transform P[c] = ((R[c][0] * p[0] + R[c][1] * p[1]) + R[c][2] * p[2]) + t[c] and O the same formula applied to origin3;
 *      without one P = p and O = origin3, the bits as they are.
 *   2. v = P - O;  L = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]).  The point is DROPPED unless L >= min_range && L <= max_range (a NaN
 *      fails; L == 0 fails, min_range being positive).  d[c] = v[c] / L.
 *   3. step = 0.5f * voxel_size;  K = (int)ceilf(tranc_dist / step) (formed on the host in these operations; at most XS_FUSE_MAX_HALF_STEPS);
 *      k_far = (int)floorf(L / step);  k_lo = carve ? -k_far : -min(K, k_far): the ray never starts behind the sensor.  k = k_lo .. K, ascending.
 *   4. Q[c] = P[c] + (float(k) * step) * d[c];  g[c] = Q[c] / voxel_size.  The sample is OUTSIDE unless g[c] >= 0 && g[c] < float(res[c]) on
 *      every axis, tested in float before any conversion;  i[c] = (int)floorf(g[c]).
 *   5. An inside sample whose voxel i equals the voxel of this ray's previous inside sample is skipped (each index is monotone in k: a ray
 *      visits a voxel once).
 *   6. C[c] = (float(i[c]) + 0.5f) * voxel_size;  sd = ((P[0] - C[0]) * d[0] + (P[1] - C[1]) * d[1]) + (P[2] - C[2]) * d[2]: the distance from
 *      the voxel centre to the point along the ray, positive in front of it;  u = sd / tranc_dist.  The sample is skipped if u < -1.0f;
 *      then u = fminf(u, 1.0f).
 *   7. q = (int)rintf((u + 1.0f) * 32768.0f), in 0 .. 65536 (ties to even);  (1ull << 40) | q is added to the voxel's word: a VISIT.
 * counts4_dev (device, never null) is INCREMENTED by {points used, points dropped, visits, samples outside}: integer atomics, one per
 * counter and workgroup.  Nothing else is written; the volume is not an argument.
 * hipErrorInvalidValue, with nothing launched and nothing written: n outside 1 .. XS_FUSE_MAX_POINTS; a null points, origin, resolution,
 * options, accumulator or counts pointer; opts->struct_bytes not sizeof(xs_fuse_opts); xs_tsdf_merge's axis rule; voxel_size or tranc_dist
 * not positive and finite; K above XS_FUSE_MAX_HALF_STEPS; an entry of the transform or the origin, min_range or max_range not finite;
 * min_range <= 0; max_range < min_range; max_range / step > 2^20.
 *
 * xs_tsdf_fuse_points_fold: one lane per voxel of planes [z0, z1) of a volume given as xs_tsdf_merge takes its destination (one pitch
 * `step` in bytes for the three arrays, byte offsets in 64 bits, the pointers at plane 0).  a = the voxel's accumulator word:
 *   a >> 40 == 0: the voxel keeps its bits, nothing is stored to it or to its word, and it does not count.
 *   otherwise, in double: m = double(a & ((1ull << 40) - 1)) / double(a >> 40);  o = float(m * 0x1p-15 - 1.0): the mean observation, one
 *      rounding to float32.  wp = the voxel's weight, ws = obs_weight.  wp == 0: value = o, grad = 0.0f.  Otherwise
 *      value = (prev * float(wp) + o * float(ws)) / float(wp + ws) and grad = (gprev * float(wp)) / float(wp + ws): the cloud carries no
 *      derivative, its observation is real.  weight = min(wp + ws, max_weight).  The word is set to 0.  The voxel counts as written.
 * *written_dev (optional, device) is INCREMENTED by the voxels written.  A row's padding, the planes outside the range and their words are
 * never touched.  A sweep thus weighs as ONE observation per voxel it touches, like a depth frame, however many of its rays pass through it.
 * hipErrorInvalidValue, with nothing launched: a null array, resolution or accumulator; xs_tsdf_merge's axis, pitch and plane-range rules;
 * max_weight outside [1, 1 << 24]; obs_weight outside [1, max_weight]. */
#define XS_FUSE_MAX_POINTS ((1 << 24) - 1)
#define XS_FUSE_MAX_HALF_STEPS 256
typedef struct xs_fuse_opts {
    unsigned struct_bytes;     /* sizeof(xs_fuse_opts) */
    float min_range;           /* metres, > 0: a shorter ray is dropped */
    float max_range;           /* metres, >= min_range: a longer ray is dropped */
    int carve;                 /* 0: the ray starts at most tranc_dist in front of the point; otherwise at the sensor, writing free space */
} xs_fuse_opts;
size_t xs_tsdf_fuse_accumulator_bytes(const int *res);
int xs_tsdf_fuse_points_accumulate(long long n, const float *points3xN_dev, const float *xform12, const float *origin3, const int *res, float voxel_size,
                                   float tranc_dist, const xs_fuse_opts *opts, unsigned long long *accumulator, unsigned long long *counts4_dev,
                                   void *stream);
int xs_tsdf_fuse_points_fold(float *value, int *weight, float *grad, size_t step, const int *res, int z0, int z1, unsigned long long *accumulator,
                             int obs_weight, int max_weight, unsigned long long *written_dev, void *stream);

/* ---- surface mesh (export; marching cubes with complex-step vertex derivatives) -------------------------------------------------------
 * No working counterpart in the reference (its extractMesh, ExtractPointCloud.cu:364-715, is never called).
 * Cube (x, y, z), x < X-1, y < Y-1, z in [z0, z1), is live when all 8 corners have weight >= min_weight and value < 0.99 and its corners
 * are neither all negative nor all non-negative (negative: value < 0).  One vertex per sign-changing edge of a live cube:
 *   vertices_dev   xyz, the point export's expression (every vertex is, bit for bit, a point xs_extract_points reports)
 *   vertex_im_dev  Im of the same expression on the (value, grad) pairs (raw: divide by the CSFD step); written only if grad != NULL
 *   normals_dev    unit central difference of the trilinear TSDF (k_extract_normals' sampling; 0 where the point export's border rule
 *                  gives 0), pointing toward increasing TSDF; written only if want_normals
 *   keys_dev       ((z * Y + y) * X + x) * 3 + axis of the edge's lower endpoint in global coordinates, axis 0/1/2 = +x/+y/+z
 * in ascending key order, and int32 index triples into them in triangles_dev, in ascending cube index ((z * Y + y) * X + x) then case
 * table order, counter-clockwise seen from the non-negative side.  The output is a function of the volume alone: bit-identical across
 * runs and with or without a sign map.  *vertex_count_host / *triangle_count_host always receive the counts found; if either exceeds its
 * capacity the call returns XS_MESH_OVER_CAPACITY and writes no output array (count-then-fill: a call with capacities 0 and NULL arrays
 * counts).  workspace: xs_mesh_workspace_bytes(res, opts).  Synchronises the stream. */
#define XS_MESH_OVER_CAPACITY (-2)
typedef struct xs_mesh_opts {
    unsigned struct_bytes;           /* sizeof(xs_mesh_opts) */
    int zs0, zs1;                    /* the arrays hold stored planes [zs0, zs1) and point at plane zs0 (whole volume: 0, 0 = res[2]) */
    int z0, z1;                      /* the cubes of planes [z0, z1) are meshed, zs0 <= z0 <= z1 <= res[2] - 1, z1 < zs1 (plane z1 is read) */
    int min_weight;                  /* corner weight gate; values below 1 mean 1 */
    int want_normals;
    const void *signmap;             /* a sign map that is a superset of the volume's negative voxels (xs_signmap_*), or NULL: bricks whose
                                        dil byte is clear are skipped without reading the volume */
    int signmap_shift;               /* its brick shift (2..6) */
} xs_mesh_opts;
size_t xs_mesh_workspace_bytes(const int *res, const xs_mesh_opts *opts);   /* opts NULL: enough for any plane range */
int xs_extract_mesh(const float *value, const int *weight, const float *grad, size_t vol_step, const int *res, float voxel_size,
                    const xs_mesh_opts *opts, float *vertices_dev, float *vertex_im_dev, float *normals_dev, unsigned long long *keys_dev,
                    size_t vertex_capacity, int *triangles_dev, size_t triangle_capacity, void *workspace, size_t *vertex_count_host,
                    size_t *triangle_count_host, void *stream);
/* host only: the edges of a case's triangles, three per triangle, -1 after the last (at most 5).  Corner c sits at (c & 1, c >> 1 & 1,
 * c >> 2 & 1) and is bit c of the case; edge e runs along axis e / 4 from the corner whose other two coordinates (x, y, z order) are the
 * bits of e % 4.  On every face the crossings are paired by that face's signs alone (an ambiguous face cuts off its negative corners). */
int xs_mesh_case_table(int cube_case, signed char out16[16]);

/* ---- ICP normal equations ----------------------------------------------------------------- */
size_t xs_icp_workspace_bytes(void);
/* zero the workspace's arrival ticket (its first 256 bytes) once after allocation; every launch leaves it zero */
int xs_icp_workspace_init(void *workspace, void *stream);
/* Device half of estimateCombined (ICP.h:24-31, ICP.cu:166-281 + 120-164): sums_dev receives 55
 * doubles — the 27 complex<double> sums in the reference's mbuf order, then the inlier count.
 * workspace replaces gbuf.  [y0, y1): pixel rows covered, 0 <= y0 <= y1 <= rows; an empty range is a launch like any other and
 * gives 55 zeros (it reads nothing outside the maps, y0 == y1 == rows included).  done_flag (optional; with sums_dev in
 * host-coherent pinned memory): the kernel stores done_seq there, system-scope release, after the
 * sums — the host may spin on it instead of copying + synchronising.  No synchronisation.
 * done_flag == XS_ICP_PUBLISH_PAIRS (xs_icp_accumulate, _real, _posted, _posted_real): sums_dev is host-coherent pinned memory of
 * XS_ICP_PAIRS_BYTES taking 55 pairs {u64 done_seq, double sum} — every sum leaves as one 16-byte store that carries its own sequence
 * word, so no completion word has to be ordered behind the sums (on the device: no wait for the stores' acknowledgement, no barrier, no
 * release store).  The host spins until all 55 sequence words equal done_seq (xs_icp_wait_pairs does); a posted launch that gave up
 * writes done_seq | 1 << 63 into the first pair's word.  Use a different done_seq for every launch on a buffer.
 * workspace (xs_icp_accumulate and every variant that takes one): its first 256 bytes must be ZERO (xs_icp_workspace_init).  Otherwise
 * no workgroup is elected last and nothing is published — sums_dev, the pairs and done_flag are not written, and the call still returns 0;
 * xs_estimate_combined and the orchestrator see the stream drain without the result and report an error instead of spinning. */
#define XS_ICP_PUBLISH_PAIRS ((unsigned long long *)(size_t)1)
#define XS_ICP_PAIRS_BYTES (55 * 16)
/* host: spin until every pair of `pairs_host` carries `seq`, then copy the 55 sums out.  0 = done, 1 = the launch gave up (its poses never
 * came), 2 = nothing within max_spins polls. */
int xs_icp_wait_pairs(const void *pairs_host, unsigned long long seq, double *sums55, long long max_spins);
int xs_icp_accumulate(const float *Rcurr18, const float *tcurr6, const float *vmap_curr, const float *nmap_curr,
                      const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                      const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres, int y0, int y1,
                      void *workspace, double *sums_dev, unsigned long long *done_flag, unsigned long long done_seq, void *stream);
/* estimateCombined with the final addition left to the host (same reference interface, ICP.h:24-31; it replaces TranformReduction,
 * ICP.cu:120-164, by a loop on the CPU that is waiting for the result anyway).  Every workgroup stores its record — 56 doubles: the 54
 * partial sums, the inlier count, a sequence word — straight into records_host (host-coherent pinned memory, xs_icp_records_bytes()
 * bytes, zero before first use) and leaves; the sequence word is written last, system-scope release.  No workspace, no ticket, no
 * completion word.  Pose: Rcurr18 / tcurr6, or both NULL with a mailbox and its sequence number (xs_icp_accumulate_posted's
 * protocol).  seq: non-zero, below 2^63, different from the previous launch's on the same buffer.
 * xs_icp_records_count: records a launch over pixel rows [y0, y1) of a cols-wide level writes.
 * xs_icp_sum_records (host only): waits for record 0 .. count - 1 in turn and adds them in that order (deterministic); sums55 = 54
 * sums + inlier count.  Returns 0; 1 if the launch reports that it gave up waiting for a posted pose; -1 after max_spins polls
 * (max_spins <= 0: wait for ever). */
size_t xs_icp_records_bytes(void);
int xs_icp_records_count(int cols, int y0, int y1);
int xs_icp_accumulate_records(const float *Rcurr18, const float *tcurr6, const void *mailbox, unsigned mailbox_seq, const float *vmap_curr,
                              const float *nmap_curr, const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                              const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres, int y0, int y1,
                              double *records_host, unsigned long long seq, void *stream);
int xs_icp_sum_records(const double *records_host, int count, unsigned long long seq, double *sums55, long long max_spins);

/* Test hook for the gate shortcut of the correspondence search: the two rejection tests of ICP.cu:232-241 use only the real
 * part of a complex square root, which the kernel settles from bounds on it unless the value sits on the threshold (then it
 * runs the square root).  Compares that decision with the full evaluation on n complex values (device memory, re / im
 * interleaved): counts_dev[0] = disagreements (must stay 0), counts_dev[1] = values that needed the square root.
 * counts_dev = two zeroed 32-bit words in device memory.  No synchronisation. */
int xs_icp_gate_selftest(const float *z2n_dev, int n, float thres, int or_equal, unsigned *counts_dev, void *stream);
/* estimateCombined with the pose posted AFTER the launch (same reference interface as above; it
 * replaces the launch latency between two iterations of KinectFusionReconstruction.cpp:187-225).
 * The call is made while the previous iteration is still running; the launch becomes resident behind
 * it, polls `mailbox` — xs_icp_mailbox_bytes() (128) bytes, 64-byte aligned, that the host can write and
 * the device read coherently (xs_icp_mailbox_alloc), zero before first use — and starts on the pixels once xs_icp_post_pose(mailbox, Rcurr18, tcurr6, mailbox_seq, 0)
 * has been called; cmd = 1 makes the launch return without touching anything (the host left the loop).
 * Several launches may be queued behind one another, with mailbox sequence numbers that increase in launch order (compared
 * as signed 32-bit distances): each waits for its own number; an abandon command (cmd = 1) posted with a LATER launch's number
 * releases every queued launch up to that one, so one post empties the queue.
 * A launch whose pose never arrives gives up after about a second and stores done_seq | 1<<63 to
 * done_flag; call xs_icp_workspace_init again after that.  One mailbox serves one stream: post
 * sequence numbers in launch order, each only after the previous launch's sums were consumed. */
size_t xs_icp_mailbox_bytes(void);
/* a zeroed mailbox where polling is cheapest: fine-grained device memory the CPU writes through the
 * large PCIe BAR (the workgroups then poll local memory), else host-coherent pinned memory */
int xs_icp_mailbox_alloc(void **mailbox, int *in_device_memory);
int xs_icp_mailbox_free(void *mailbox, int in_device_memory);
int xs_icp_accumulate_posted(const void *mailbox, unsigned mailbox_seq, const float *vmap_curr, const float *nmap_curr,
                             const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                             const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres, int y0,
                             int y1, void *workspace, double *sums_dev, unsigned long long *done_flag, unsigned long long done_seq,
                             void *stream);
/* host: writes the mailbox (four 32-byte sectors, each its sequence word + payload: two 64-byte lines).  On a CPU with MOVDIR64B each line is one direct 64-byte
 * store; otherwise payload, store fence, sequence words, store fence.  One post per posted launch, from one host thread per mailbox. */
void xs_icp_post_pose(void *mailbox_host, const float *Rcurr18, const float *tcurr6, unsigned mailbox_seq, int cmd);
/* xs_icp_accumulate / xs_icp_accumulate_posted reading the current-frame maps' real parts from float planes (xs_create_vnmaps_real;
 * 3 x rows rows of cols floats, pitch real_step bytes) instead of the complex maps, whose imaginary parts must be zeros — true for
 * maps made from a real depth image, i.e. always in this pipeline.  Half the bytes of the kernel's current-frame reads; the same sums
 * (an imaginary part that was -0 in the complex map is +0 here).  vmap_curr / nmap_curr may be NULL. */
int xs_icp_accumulate_real(const float *Rcurr18, const float *tcurr6, const float *vmap_curr, const float *nmap_curr,
                           const float *vmap_curr_real, const float *nmap_curr_real, size_t real_step, const float *Rprev_inv18,
                           const float *tprev6, const float *intr4, const float *vmap_g_prev, const float *nmap_g_prev, size_t map_step,
                           int rows, int cols, float distThres, float angleThres, int y0, int y1, void *workspace, double *sums_dev,
                           unsigned long long *done_flag, unsigned long long done_seq, void *stream);
int xs_icp_accumulate_posted_real(const void *mailbox, unsigned mailbox_seq, const float *vmap_curr, const float *nmap_curr,
                                  const float *vmap_curr_real, const float *nmap_curr_real, size_t real_step, const float *Rprev_inv18,
                                  const float *tprev6, const float *intr4, const float *vmap_g_prev, const float *nmap_g_prev,
                                  size_t map_step, int rows, int cols, float distThres, float angleThres, int y0, int y1, void *workspace,
                                  double *sums_dev, unsigned long long *done_flag, unsigned long long done_seq, void *stream);
/* One whole ICP iteration without leaving the device: estimateCombined followed by the pose update
 * the reference's host performs before the next launch (KinectFusionReconstruction.cpp:203-224:
 * A.real().determinant() gate, complex<double> llt().solve, cast to complex<float>, AngleAxis
 * Z*Y*X, tcurr = Rinc*tcurr + tinc, Rcurr = Rinc*Rcurr).  pose_state: xs_icp_pose_state_bytes()
 * (128) bytes of device memory laid out {float R[18]; float t[6]; int status; int iters; double det;
 * double pad[2]}.  With Rcurr18 / tcurr6 given the launch starts from them (first iteration of a
 * frame), with both NULL from the state the previous launch on the stream left.  status: 0 ok,
 * 1 |det| < 1e-15, 2 NaN det — once non-zero the following launches return at once, which is where
 * the reference leaves PoseEstimate.  sums_dev: device memory, as above.  sums_host / pose_state_host
 * (optional, host-coherent pinned memory) receive a copy of the 55 sums and of the state after every
 * solve; done_flag / done_seq as above (published after both).  Each call enqueues the reduction and a
 * one-workgroup solve kernel; the iterations of a frame queue back to back: no synchronisation, one
 * host wait per frame instead of one per iteration. */
size_t xs_icp_pose_state_bytes(void);
int xs_icp_iterate(const float *Rcurr18, const float *tcurr6, const float *vmap_curr, const float *nmap_curr,
                   const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                   const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres, void *workspace,
                   double *sums_dev, double *sums_host, void *pose_state, void *pose_state_host, unsigned long long *done_flag,
                   unsigned long long done_seq, void *stream);
/* estimateCombined(...) whole: accumulate, wait for the launch (the host spins on a pinned record the kernel's last workgroup writes: everything
 * before it on the stream has completed when the call returns — what the reference's device synchronisation gives, without the stream drain),
 * unpack into the symmetric A (36 complex<double>, A[i*6+j] = A[j*6+i]) and b (6).  sums_dev: optional device copy of the 55 doubles.
 * A launch that fails returns its HIP error; one that completes without publishing (a workspace whose ticket is not zero, see
 * xs_icp_workspace_init) returns hipErrorLaunchTimeOut about a millisecond after the stream drained.
 *                                                                              ICP.cu:365-429 */
int xs_estimate_combined(const float *Rcurr18, const float *tcurr6, const float *vmap_curr, const float *nmap_curr,
                         const float *Rprev_inv18, const float *tprev6, const float *intr4, const float *vmap_g_prev,
                         const float *nmap_g_prev, size_t map_step, int rows, int cols, float distThres, float angleThres,
                         void *workspace, double *sums_dev, double *A72_host, double *b12_host, long long *inliers, void *stream);
/* ICP.cu:419-428 on host data: 27 (re, im) sums -> A[36], b[6] */
void xs_icp_unpack(const double *sums54, double *A72, double *b12);

/* ---- DeviceArray complex math over arrays -------------------------------------------------- */
/* Experiments/test_CSFD/main.cpp:18-86 over arrays: which 0 mul 1 div 2 exp 3 sin 4 pow(.,3);
 * our 0 = *_raw, 1 = *_our. */
int xs_csfd_array_op(int which, int our, const float *a, const float *b, float *out, long n, void *stream);
/* f1(x, y) = (x + y)^2 in dual-complex arithmetic (test_CSFD/main.cpp:8-11) */
int xs_dcsfd_f1(const float *x, const float *y, float *out, long n, void *stream);
/* elementwise complex<float> (dual = 0) / d_complex<float> (dual = 1) operator tables
 * (cuda_complex.hpp:100-881, cuda_double_complex.hpp:137-260); op codes listed in DESIGN.md */
int xs_complex_table(int dual, int op, const float *a, const float *b, float *out, long n, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* XSLAM_AMD_H */
