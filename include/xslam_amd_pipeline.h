/* xslam_amd_pipeline.h — C ABI of the host orchestrator (libxslam_host.so): the C++ class
 * KinectFusionReconstruction (x-slam_amd/host/, mirroring
 * XKinectFusion/include/KinectFusionReconstruction.h:19-174) behind an opaque handle, for
 * callers that are not C++ (bench.py, the parity tests).  Config is the reference's flat YAML
 * (Experiments/test_xkinect_fusion/configs/ICL_traj2.yaml) passed as text, plus the optional
 * keys csfd_seed_row / csfd_seed_col / csfd_seed_h.
 * 4x4 complex matrices cross as 32 floats, row-major (re, im) pairs.  Errors inside the
 * pipeline print and exit(-1), as the reference's cudaSafeCall does (Common/include/cx.h:124-130).
 */
#ifndef XSLAM_AMD_PIPELINE_H
#define XSLAM_AMD_PIPELINE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Host DoubleComplex (x-slam_amd/host/DoubleComplex.h, mirroring DeviceArray/include/DoubleComplex.h:15-95)
 * over arrays of n groups (re.re, re.im, im.re, im.im).  op: 0 add 1 sub 2 mul 3 div 4 sqrt 5 abs 6 exp
 * 7 log 8 sin 9 cos 10 pow(x, y.re.re) 11 f1(x, y) = (x + y)^2 12 conj 13 norm 14 (x > y, x < y).  CPU only. */
int xs_host_double_complex_table(int op, long n, const float *a, const float *b, float *out);
/* Host instantiation of the complex<float> operators (x-slam_amd/csrc/xs_complex.h is host + device, like
 * DeviceArray/include/cuda_complex.hpp:12-16): n interleaved (re, im) pairs, op codes of xs_complex_table
 * (include/xslam_amd.h).  Returns 0, -1 for a bad op.  CPU only. */
int xs_host_complex_table(int op, long n, const float *a, const float *b, float *out);

/* Flat "key: value" config reader (x-slam_amd/host/flat_yaml.hpp; stands in for yaml-cpp's
 * config["k"].as<T>() of KinectFusionReconstruction.cpp:12-72): copies the value of key into out.
 * Returns its length, -1 if the key is absent.  CPU only. */
int xs_flat_yaml_get(const char *yaml_text, const char *key, char *out, int capacity);

/* hipStream_t (as void*) every later call enqueues on; NULL = default stream */
void xs_kf_set_stream(void *stream);
/* KinectFusionReconstruction() + SetYamlParameters(config)     KinectFusionReconstruction.cpp:4-73
 * returns NULL (and prints) on a missing key */
void *xs_kf_create(const char *yaml_text);
/* Sharded instance (the reference is single-GPU): rank r of count owns the z planes
 * [r*Z/count, (r+1)*Z/count) (+ 6 halo planes each side) and the pixel rows [r*H/count, ...) of
 * every ICP level.  collective(user, op, dev_ptr, count) must all-reduce dev_ptr in place over
 * the ranks, ordered on the current stream: op 0 = sum of doubles (the 27 complex<double>
 * normal-equation sums + inlier count), 1 = min of int32 (first raycast event per pixel),
 * 2 = sum of int32 (the owned-pixel counts of the raycast composite; with shard_composite_gather: false the vertex / normal maps as bit
 * patterns), 3 = gather of variable-size parts: dev_ptr is then a HOST array of count + 2 64-bit words — [0] the device buffer's address,
 * [1 + r] .. [2 + r] the byte range of rank r's part in it — this rank's part is in place when the call is made, every rank's when the
 * operation has completed on the stream (count = the number of ranks; the parts are whole 52-byte entries).
 * xs_kf_download_volume then returns the stored planes only (xs_kf_shard_planes). */
void *xs_kf_create_sharded(const char *yaml_text, int rank, int count, void (*collective)(void *user, int op, void *dev_ptr, long n),
                           void *user);
void xs_kf_shard_planes(void *kf, int *owned2, int *stored2);
void xs_kf_destroy(void *kf);
/* gt_poses (camera-to-world) for flag_use_gtPose: n matrices of 32 floats   .h:36, .cpp:239-247 */
void xs_kf_set_gt_poses(void *kf, int n, const float *c2w32);
/* ProcessFrame(const DeviceArray2D<ushort>& depth_frame_d)     .cpp:147-159
 * depth_dev: u16 millimetres resident in device memory, row pitch step_bytes.  Returns 1, or 0
 * when the alignment failed (frame_id is then not advanced, as in the reference). */
int xs_kf_process_frame(void *kf, const uint16_t *depth_dev, size_t step_bytes);
/* Look-ahead (no reference counterpart: main.cpp:50-58 handles one frame at a time): the device depth image the NEXT xs_kf_process_frame
 * call will be given — it must stay unchanged until that call.  Its maps (bilateral filter, depth pyramid, vertex / normal maps, scaled depth) are then built
 * during the current frame's ICP loop, when the GPU is mostly idle, into a second set of buffers.  A call with any other image prepares its own maps as always; results are the same bits
 * either way.  Call before xs_kf_process_frame of the current frame. */
void xs_kf_hint_next_frame(void *kf, const uint16_t *depth_dev, size_t step_bytes);
/* the reference demo's upload + ProcessFrame (main.cpp:50-58): host buffer, dense rows.  The frame is copied
 * asynchronously on the pipeline's second stream (through a pinned staging buffer unless depth_host is
 * itself pinned), where the map preparation follows it without a host wait. */
int xs_kf_process_frame_host(void *kf, const uint16_t *depth_host);
/* the next of two host-pinned staging buffers (depth_width x depth_height u16): decode a frame straight into
 * it and pass it to xs_kf_process_frame_host — no staging copy.  Blocks only if the copy out of that buffer
 * two frames ago has not finished. */
uint16_t *xs_kf_ingest_buffer(void *kf);
/* getCamera2Volume()  .h:137: world2volume * world2camera^-1 of the latest pose, 32 floats */
void xs_kf_get_camera2volume(void *kf, float *out32);
/* Pose refinement against the map (BASELINE config 5): Gauss-Newton on the residual of ComputeLocalTsdf_hessian
 * with the Jacobian from first-order CSFD — six poses seeded with i*1e-7 along the generators of
 * camera2volume <- se3Exp(xi) * camera2volume, one pass over the volume (xs_tsdf_gauss_newton_terms); a sharded
 * rank evaluates its slab and the sums are all-reduced.  gauss_newton_terms: out29 = J^T J upper triangle (21),
 * J^T r (6), sum r^2, count.  relocalize: `iterations` steps of (J^T J + damping * diag) delta = -J^T r from c2v32
 * (updated in place); loss_out (optional, iterations + 1 doubles): mean squared residual before each step and at
 * the end.  Both return 1, or 0 when there is nothing to align to. */
int xs_kf_gauss_newton_terms(void *kf, const uint16_t *depth_dev, size_t step_bytes, const float *c2v32, double *out29);
int xs_kf_relocalize(void *kf, const uint16_t *depth_dev, size_t step_bytes, float *c2v32, int iterations, float damping, double *loss_out);
/* Batched relocalisation against the current map: xs_kf_relocalize for each of `frames` depth images (device pointers depth_dev[f], one
 * step_bytes) from c2v32xF + 32 f (refined in place), all frames of a pass in one band-index launch (chunks of XS_BAND_MAX_FRAMES; DESIGN.md
 * section 4.15).  The band index of the owned planes is built on first use and rebuilt after anything wrote the volume (integrate,
 * loadCheckpoint, xs_kf_volume_ptr(kf, 0, .), xs_kf_rebuild_sign_map).  Frame f's ok_out[f], pose and losses (loss_out + f (iterations + 1);
 * NULL: no final loss pass, as xs_kf_relocalize) are bit-identical to what xs_kf_relocalize returns for that frame alone.  Returns the
 * number of frames that succeeded (-1: bad arguments). */
int xs_kf_relocalize_batch(void *kf, int frames, const uint16_t *const *depth_dev, size_t step_bytes, float *c2v32xF, int iterations, float damping,
                           double *loss_out, int *ok_out);
/* The exact pose Hessian of the map-alignment loss L = sum r^2 and Newton relocalisation.  One launch of
 * xs_tsdf_pose_hessian_band over the band index (built as for xs_kf_relocalize_batch) evaluates 21 dual-complex seeded poses per frame.
 * pose_hessian_terms: out29 = H upper triangle (21, row-major: d2L / dtheta_a dtheta_b, already divided by h^2), g (6: dL / dtheta_a,
 * divided by h), sum r^2, count — theta the twist of camera2volume <- se3Exp(theta) * camera2volume.  Returns 1, or 0 without a volume.
 * relocalize_newton / relocalize_newton_batch: xs_kf_relocalize / xs_kf_relocalize_batch with the step (H + damping * diag H) delta = -g;
 * where that system is not positive definite the frame takes the Gauss-Newton step for that iteration, and fallbacks_out (optional; one int
 * per frame) counts those iterations.  Results per frame do not depend on the batch.  Loss history and return values as their counterparts'. */
int xs_kf_pose_hessian_terms(void *kf, const uint16_t *depth_dev, size_t step_bytes, const float *c2v32, double *out29);
int xs_kf_relocalize_newton(void *kf, const uint16_t *depth_dev, size_t step_bytes, float *c2v32, int iterations, float damping, double *loss_out,
                            int *fallbacks_out);
int xs_kf_relocalize_newton_batch(void *kf, int frames, const uint16_t *const *depth_dev, size_t step_bytes, float *c2v32xF, int iterations,
                                  float damping, double *loss_out, int *ok_out, int *fallbacks_out);
/* The host's side of a Newton pass.  CPU only.  seeded_poses: the 21 dual-complex volume-to-camera poses of camera2volume c2v32 (pair (a, b),
 * a <= b, row-major; 36 + 12 floats each, the layout of xs_tsdf_pose_hessian_band); returns 0.  newton_step: s29 as pose_hessian_terms
 * returns it; solves (H + damping * diag H) delta = -g by Cholesky and applies c2v32 <- se3Exp(delta) * c2v32.  Returns 0 when the step was
 * taken, -1 (c2v32 untouched) when count < 6 or the system is not positive definite. */
int xs_host_newton_seeded_poses(const float *c2v32, float *R36x21, float *t12x21);
int xs_host_newton_step(const double *s29, double damping, float *c2v32);
/* Global relocalisation: the camera is lost and there are pose hypotheses.
 * score_poses: the real-valued alignment loss of one depth frame at `poses` camera2volume hypotheses c2v32xP + 32 p, in one launch of
 * xs_tsdf_score_poses_band over the band index (built as for xs_kf_relocalize_batch) per chunk of XS_SCORE_MAX_POSES; out2xP + 2 p =
 * {sum loss, count} at the real part of inverse(c2v) — what xs_compute_local_tsdf_loss gives for that pose on the dense map: the count
 * exactly, the sum within 8 * 2^-24 of it.  In shard mode the sums are all-reduced.  Returns 1, 0 without a volume, -1 on bad arguments.
 * relocalize_global: scores the candidates, keeps the min(keep, poses) with the highest truncated-quadratic inlier score S = count - sum loss
 * (ties: the lower index), refines them with xs_kf_relocalize_batch's loop (`iterations`, `damping`, the same depth in every slot), scores
 * the refined poses and writes to best_c2v32 the one with the highest S among those whose loop ended ok.  report8 = {the winner's candidate
 * index, its S before refinement, its S after, sum loss after, count after, how many of the kept ended ok, band voxels in the index, 0}.
 * Returns 1; 0 when none of the kept ended ok (best_c2v32 untouched, report8[0] = -1); -1 on bad arguments. */
int xs_kf_score_poses(void *kf, const uint16_t *depth_dev, size_t step_bytes, int poses, const float *c2v32xP, double *out2xP);
int xs_kf_relocalize_global(void *kf, const uint16_t *depth_dev, size_t step_bytes, int poses, const float *c2v32xP, int keep, int iterations,
                            float damping, float *best_c2v32, double *report8);
/* Next best view: where should the camera go next?
 * score_views: what the camera would see from each of `poses` hypothetical camera2volume poses c2v32xP + 32 p (the layout xs_kf_score_poses
 * takes; the real parts are used): a lattice of rays per pose marched through the observation grid of the volume — two bits per voxel,
 * unknown / free / occupied at weight gate min_weight (below 1 means 1), allocated on first use and rebuilt after anything wrote the volume
 * or when min_weight changes — in one launch of xs_score_views (xslam_amd.h: the contract) per chunk of XS_VIEW_MAX_POSES.  out4xP + 4 p =
 * {unknown, free, hits, frontier} samples of pose p.  opts: an xs_view_opts of xslam_amd.h, or NULL for the defaults (80 x 60 rays of the
 * level-0 camera, depths 0.2 .. 5.0 in steps of a voxel).  Returns 1, 0 without a volume, -1 on bad arguments or options, -2 in shard mode
 * (nothing is done: occlusion along a ray is not additive over z-slabs, and a composite like the raycast's is not built).
 * next_best_view: scores the poses and returns the index of the one with the most unknown samples among those with hits >= min_hits (a
 * view with no known surface in it cannot be tracked, so it cannot win); ties go to the lower index; -1 when no pose qualifies or there is
 * no volume, -2 in shard mode, -3 on bad arguments or options.  out4xP (optional) receives the counts. */
struct xs_view_opts;
int xs_kf_score_views(void *kf, int poses, const float *c2v32xP, const struct xs_view_opts *opts, int min_weight, unsigned *out4xP);
int xs_kf_next_best_view(void *kf, int poses, const float *c2v32xP, const struct xs_view_opts *opts, int min_weight, unsigned min_hits,
                         unsigned *out4xP);
/* Clearance and reachability of candidate views: can the camera be at a candidate, and get there?
 * clearance_field: the field of xs_clearance_build (xslam_amd.h: the contract) over the observation grid at weight gate min_weight, R =
 * max_radius_vox (1 .. 255), unknown_blocks 0 or 1: host_out[(z * Y + y) * X + x] = min(d^2, R^2) to the nearest obstacle voxel.
 * reachable: the body's radius becomes rv = radius_m / voxel_size (a float32 divide), r2 = max(1, (int)ceilf(rv * rv)), R the smallest integer
 * with R * R >= r2 (bad arguments if R exceeds 255).  The start is the real translation of start_c2v32 (NULL: the current camera2volume),
 * its voxel snapped to the nearest passable voxel (FREE and field >= r2) within snap_vox (0 .. 16; ties as xs_reach_query breaks them) — the
 * camera's own voxel is usually UNKNOWN, the sensor observes nothing at its own centre.  No such voxel: nothing is reachable, which is a
 * result.  The known free space the body fits in is flooded from there; reachable[p] = 1 iff the centre voxel of pose c2v32xP + 32 p (not
 * snapped) was reached, clear2[p] the field's value there (0 outside the volume).  The field, the flood and the grid are cached and
 * redone when the volume, min_weight, unknown_blocks, R, r2 or the snapped seed change.
 * Both return 1 when they ran, 0 without a volume, -1 on bad arguments, -2 in shard mode (nothing is done: distance and connectivity are
 * not additive over z-slabs, and a halo exchange is not built).
 * next_reachable_view: xs_kf_next_best_view's scoring and rule restricted to the candidates reachable from the current camera;
 * `reachable` (optional) receives the flags.  The index, -1 when no reachable pose qualifies or there is no volume, -2 in shard mode, -3 on
 * bad arguments or options.  xs_kf_next_best_view itself and its results do not change. */
int xs_kf_clearance_field(void *kf, int max_radius_vox, int unknown_blocks, int min_weight, uint16_t *host_out);
int xs_kf_reachable(void *kf, const float *start_c2v32_or_null, float radius_m, int snap_vox, int unknown_blocks, int min_weight, int P, const float *c2v32xP,
                    unsigned char *reachable, unsigned short *clear2);
int xs_kf_next_reachable_view(void *kf, int poses, const float *c2v32xP, const struct xs_view_opts *opts, int min_weight, unsigned min_hits, unsigned *out4xP,
                              float radius_m, int snap_vox, int unknown_blocks, unsigned char *reachable);
/* Travel cost and shortest collision-free path to a candidate view: how far is it, and which way?  The field of
 * xs_travel_build (xslam_amd.h: the contract; the <3, 4, 5> chamfer metric over the reached voxels without corner cutting, a unit is a third
 * of a voxel edge) is built from the snapped start of xs_kf_reachable, whose start arguments all three calls share, up to the limit
 * 65534 for max_travel_m <= 0 or not finite, otherwise min(65534, (int)floorf(3 * max_travel_m / voxel_size)) in float32.
 * travel: xs_kf_reachable plus travel3[p], the uint16 cost at the centre voxel of pose p (not snapped), 65535 where unreachable or beyond
 * the limit.  Returns as xs_kf_reachable does.
 * path_to: the number of voxels of the path from the start to the centre voxel of target_c2v32, START FIRST AND TARGET LAST; voxels3 (int32)
 * and points3 (float32, the voxel centres (v + 0.5) * voxel_size in volume coordinates) are optional.  0 when the target is not reached (or
 * beyond the limit, or there is no volume), -1 on bad arguments (capacity < 1 among them), -2 in shard mode, -4 with nothing written when the
 * path is longer than `capacity`; *needed_out (optional) receives the path's length whenever a walk ran.
 * next_view_by_travel: xs_kf_next_best_view's scoring; among the poses with a cost and hits >= min_hits the one with the largest
 * unknown / (travel + bias3), bias3 = max(1, (int)ceilf(3 * bias_m / voxel_size)), compared exactly in 64-bit integers, ties to the lower
 * index.  bias_m (>= 0, finite) is the fixed cost of taking any view at all.  travel3_out (optional) receives the costs.  Returns as
 * xs_kf_next_reachable_view does.  The field is cached and redone when the flood or the limit change.  In shard mode all three return -2
 * and do nothing.  xs_kf_next_best_view, xs_kf_reachable, xs_kf_next_reachable_view and their results do not change. */
int xs_kf_travel(void *kf, const float *start_c2v32_or_null, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m, int P,
                 const float *c2v32xP, unsigned char *reachable, unsigned short *clear2, unsigned short *travel3);
int xs_kf_path_to(void *kf, const float *start_c2v32_or_null, float radius_m, int snap_vox, int unknown_blocks, int min_weight, float max_travel_m,
                  const float *target_c2v32, int capacity, int *voxels3, float *points3, int *needed_out);
int xs_kf_next_view_by_travel(void *kf, int poses, const float *c2v32xP, const struct xs_view_opts *opts, int min_weight, unsigned min_hits, unsigned *out4xP,
                              float radius_m, int snap_vox, int unknown_blocks, float max_travel_m, float bias_m, unsigned short *travel3_out);
/* Frontier clusters and the views proposed from them: where should the camera go next, with no candidates from
 * the caller?  The frontier voxels of the observation grid at min_weight (FREE with an UNKNOWN face neighbour) are labelled into clusters
 * (26-adjacency within cells of `cell` voxels: 0 for the whole volume, otherwise a multiple of 8 in 8 .. 65528; xslam_amd.h: the contract).
 * frontiers: the records {label, count, sum x, sum y, sum z, packed min, packed max, 0} of the clusters with count >= min_size, ascending by
 * label, into records8 (capacity x 8 uint64; may be null when capacity is 0) and their number into *count_out.  A record's centroid in
 * metres is, per axis, ((float)((double)sum / (double)count) + 0.5f) * voxel_size.
 * propose_views: floods as xs_kf_reachable does from the current camera (its start snapped within start_snap_vox), takes those clusters and
 * for each the views_per_cluster (1 .. 4096) standpoints p_j = centroid + standoff_m * d_j, d_j the unit vector of the Halton pair
 * (u, v) = (bases 2 and 3, index j + 1) with z = 1 - 2 u and phi = 2 pi v.  Each standpoint is snapped to the nearest REACHED voxel within
 * snap_vox (0 .. 16) by xs_reach_query's rule; those that find none are dropped, and so is one whose voxel an earlier standpoint of the same
 * cluster gave.  Each survivor yields the pose at its voxel's centre (v + 0.5f) * voxel_size whose optical axis (third column) points at the
 * centroid and whose image-down axis is as close as orthogonality allows to the current camera's y axis (its x axis when y is within 8.1
 * degrees of the view direction): c2v32xP_out (capacity x 32 floats, zero imaginary parts), cluster_out (capacity ints, the index into
 * the list frontiers returns for the same cell, min_size and min_weight) and *count_out.  floorf(centre / voxel_size) is the voxel again,
 * so xs_kf_reachable and xs_kf_travel call every proposed pose reachable.
 * Both return 1 when they ran, 0 without a volume, -1 on bad arguments, -4 with the needed count in *count_out and nothing else written when
 * capacity is too small, -2 in shard mode, doing nothing.  Mask, labels and records are cached and redone when the volume, min_weight or
 * cell change.  No other call's results change. */
int xs_kf_frontiers(void *kf, int cell, unsigned long long min_size, int min_weight, int capacity, unsigned long long *records8, int *count_out);
int xs_kf_propose_views(void *kf, float radius_m, int start_snap_vox, int unknown_blocks, int min_weight, int cell, unsigned long long min_size,
                        int views_per_cluster, float standoff_m, int snap_vox, int capacity, float *c2v32xP_out, int *cluster_out, int *count_out);
/* band voxels in the relocalisation index as last built (0 before the first batch) */
long long xs_kf_relocalization_index_voxels(void *kf);
/* ExportPointCloud(max_buffer)  .cpp:334-372 (+ CPointCloud::exportPly, main.cpp:78-80): zero-crossing points of
 * the TSDF with normals, at most max_buffer; xyz triples into the host arrays (either may be NULL); returns
 * the number of points.  A sharded rank exports the planes it owns.  export_ply writes the reference's
 * ascii format (x y z nx ny nz) and returns the number of points, -1 if the file cannot be opened. */
long long xs_kf_export_point_cloud(void *kf, int max_buffer, float *points_host, float *normals_host);
long long xs_kf_export_ply(void *kf, int max_buffer, const char *filename);
/* ExportMesh (no working counterpart in the reference; xs_extract_mesh in xslam_amd.h): the marching-cubes mesh of the TSDF with
 * corner weight gate min_weight (1 = every observed voxel).  Returns the vertex count and sets *triangle_count and *has_im (1 while a
 * CSFD seed is active: vertex_im then holds Im of every vertex, raw — divide by csfd_seed_h).  The arrays (any may be NULL: vertices,
 * normals, vertex_im xyz triples; edge_keys; triangles index triples) are filled only if both counts fit the capacities: count with
 * capacities 0, allocate, call again.  A sharded rank meshes the cubes of the planes it owns.  export_mesh_ply writes binary little-endian
 * PLY (vertex x y z nx ny nz [dx dy dz: vertex_im, raw], face list uchar int vertex_indices); returns the vertex count, -1 if the file
 * cannot be written. */
long long xs_kf_export_mesh(void *kf, int min_weight, long long vertex_capacity, long long triangle_capacity, float *vertices_host,
                            float *normals_host, float *vertex_im_host, unsigned long long *edge_keys_host, int *triangles_host,
                            long long *triangle_count, int *has_im);
long long xs_kf_export_mesh_ply(void *kf, const char *filename);
void xs_kf_synchronize(void *kf);

int xs_kf_frame_id(void *kf);
int xs_kf_num_poses(void *kf);                                   /* world2camera_record.size() */
void xs_kf_get_world2camera(void *kf, int idx, float *out32);    /* idx < 0 counts from the back */
float xs_kf_tranc_dist(void *kf);
long long xs_kf_last_updated_voxels(void *kf);                   /* U of the last integrate */
long long xs_kf_last_raycast_hits(void *kf);
/* per ICP iteration of the last frame: 54 sums (27 x re, im) + inlier count; returns #doubles */
int xs_kf_icp_log(void *kf, double *out, int capacity);

/* dense host copies (X*Y*Z each; any pointer may be NULL)   TsdfVolume.cpp:64-77 */
int xs_kf_download_volume(void *kf, float *value, int *weight, float *grad);
/* which: 0 depths_curr 1 vmaps_curr 2 nmaps_curr 3 vmaps_g_prev 4 nmaps_g_prev; out: planes x
 * rows x cols x (re, im), dense */
int xs_kf_download_map(void *kf, int which, int level, float *out);
/* device pointers + pitch of the live arrays: which 0 value 1 weight 2 grad.  Asking for the value array (which 0) marks the ray march's
 * sign map stale: it is rebuilt from the volume in front of the next raycast (one pass over the value array), so a caller that writes
 * values through the pointer needs no further call; a caller that only reads pays that pass once per request. */
void *xs_kf_volume_ptr(void *kf, int which, size_t *step_bytes);

/* HIP-event timing.  level 0: off.  1: the integrate kernel's own event pair (stage 3) and the per-frame
 * counters — nothing extra on the stream between kernels.  2: an event pair around every stage too
 * (0 surface 1 icp 2 scale 3 integrate 4 raycast 5 resize); every record is a packet the next kernel
 * queues behind, so a frame is ~10 % slower at level 2 than at level 1. */
void xs_kf_set_profiling(void *kf, int level);
void xs_kf_stage_times(void *kf, double *ms6, long long *calls6);
/* voxels written / raycast hits summed over the frames processed with profiling on */
void xs_kf_cumulative_counters(void *kf, long long *updated, long long *hits);
void xs_kf_reset_stage_times(void *kf);
/* Host wall clock of the ICP loop per pyramid level (index = level, 0 = full resolution; index 3 = the first iteration of each frame,
 * kept apart because it also waits for the stream to drain the previous frame's tail): microseconds summed over the iterations run since
 * the last xs_kf_reset_stage_times, and their count — the period from one iteration's sums arriving to the next one's (kernel, completion
 * word, 6x6 solve, pose post).  ICP.cu:395-417 is a launch + device sync + copy per iteration.  Always on. */
void xs_kf_icp_iteration_times(void *kf, double *us4, long long *calls4);
/* Host wall clock of a tracked frame's tail since the last xs_kf_reset_stage_times, microseconds summed over *frames frames: us4[0] the last ICP
 * sums seen -> IntegrateFrame entered (6x6 solve, pose algebra), [1] entered -> the integrate launch call (transforms, cover test), [2] the
 * launch call itself, [3] its return -> the raycast launch's return. */
void xs_kf_tail_host_times(void *kf, double *us4, long long *frames);
/* The Gauss-Newton passes xs_kf_relocalize has run since the last reset: *pass_us = host wall clock summed over *passes passes (from a loop's
 * first kernel enqueued to its last sums seen: kernel + the record's way to the host + the 6x6 solve + the six pose inversions + the post);
 * *kernel_ms / *kernel_calls = the kernels' own durations, of passes run with profiling on (xs_kf_set_profiling >= 1: an event pair around each).
 * reset != 0 zeroes the four.  pass - kernel is what the host's side of a pass costs (bench.py: workloads.reloc.host_us_per_pass). */
void xs_kf_gn_times(void *kf, double *pass_us, long long *passes, double *kernel_ms, long long *kernel_calls, int reset);
/* The host's side of a Gauss-Newton pass as the DEVICE sees it: *poll_us = microseconds the kernels that were enqueued ahead waited for their poses (from
 * resident — i.e. the previous pass's kernel gone — to poses seen, on the device's 100 MHz clock), summed over *poll_passes such passes since the last
 * reset: the record's way to the host, the solve, the six pose inversions, the post and its way back.  No events involved. */
void xs_kf_gn_poll_times(void *kf, double *poll_us, long long *poll_passes, int reset);
/* YAML gn_post_pose at run time (0: every Gauss-Newton pass launched with its poses as arguments, after the solve — a kernel's event pair then times
 * the kernel alone; a pass enqueued ahead also spends the host's turnaround polling its mailbox inside the pair) */
void xs_kf_set_gn_post_pose(void *kf, int on);
/* Test aids.  Start the ICP launch sequence numbers at v (exercises the 2^32 wrap of the mailbox numbers); make the determinant gate of
 * iteration n (0-based, over all levels) of the next alignment fail as for a singular system (KinectFusionReconstruction.cpp:203-210). */
void xs_kf_debug_set_icp_sequence(void *kf, unsigned long long v);
void xs_kf_debug_fail_icp_iteration(void *kf, int n);
/* test aid: a random host sleep of [min_us, max_us] microseconds in front of every ICP pose post (0, 0 = none): a slow host must neither
 * time a resident launch out nor change a pose */
void xs_kf_debug_post_delay(void *kf, int min_us, int max_us);
/* Rebuilds the sign map of the ray march (xslam_amd.h) from the volume now (in shard mode: from the planes this rank stores, on every
 * rank).  xs_kf_volume_ptr(kf, 0, .) schedules the same in front of the next raycast and loadCheckpoint does it itself, so this is
 * only for a caller that kept the pointer and wrote through it again later.  No-op with raycast_sign_map: false. */
void xs_kf_rebuild_sign_map(void *kf);
/* shard mode: bytes this rank has received through the raycast composite's collectives since creation (a ring all-reduce of S bytes over N
 * ranks counted as 2 (N - 1) / N x S, the gather of the owned pixels as the other ranks' parts) */
long long xs_kf_composite_bytes(void *kf);
/* How often the brick list and box classes decided ahead of a frame's final pose (behind its last ICP launch) held for that pose: counts4[0]
 * neither (everything classified again), [1] the list only (the boxes decided again with the final pose), [3] both. */
void xs_kf_list_cover_counts(void *kf, long long *counts4);

/* volume checkpoint (value + grad + weight + poses)   cf. saveTSDFVolume, .cpp:438-447 */
/* The version of the volume's contents: incremented by everything that writes the volume (a frame, a merge, a loaded checkpoint,
 * xs_kf_volume_ptr of the value array); the cached band index and planning maps are rebuilt when it has moved.  Calls that only read the
 * map (relocalisation, export, xs_kf_align_map on either instance) leave it alone. */
long long xs_kf_volume_generation(void *kf);
int xs_kf_save_checkpoint(void *kf, const char *path);
int xs_kf_load_checkpoint(void *kf, const char *path);
int xs_kf_save_tsdf_volume(void *kf, const char *path);
/* The brick-sparse checkpoint XSTSDF3 ("Checkpoint formats"), lossless.  The save above writes the dense
 * XSTSDF2 as before; this one classifies and compacts the volume on the device and streams it through one pinned staging buffer, never holding
 * the whole volume on the host.  A rank of a sharded run saves its own planes.  The load above and every *_checkpoint call take either format:
 * they look at the magic.  stats12 (optional): bricks, the bricks of classes 0 .. 7, payload words, file bytes, gather chunks.
 * Return 0; -1 without a volume or when the file cannot be written. */
int xs_kf_save_checkpoint_sparse(void *kf, const char *path, unsigned long long *stats12);
/* The staging buffer of sparse saves and loads, in 32-bit words: sets it when words >= 1536 (one brick at its largest; 0 leaves it alone) and
 * returns the value in effect, by default 16 Mi words = 64 MiB; -1 for a value between.  Pinned host memory and the device buffer of a chunk are
 * bounded by it whatever the volume's size. */
long long xs_kf_checkpoint_staging_words(void *kf, unsigned long long words);
/* What a checkpoint file of either format holds, without a GPU and without reading a payload: the header, and for XSTSDF3 the class bytes, under
 * the format's full validation (XSTSDF2: geometry, pose count, exact length; XSTSDF3: pack_validate of x-slam_amd/host/pack_host.hpp).
 * out32: 0 format version (2 or 3); 1 valid (1 / 0); 2 .. 4 res; 5 voxel size; 6 truncation distance; 7 frame_id; 8 n_poses; 9, 10 zs0, zs1;
 * 11, 12 shard rank and count; 13 brick edge; 14 .. 16 nbx, nby, nbz; 17 nbricks; 18 .. 25 bricks of classes 0 .. 7; 26 payload words (XSTSDF2:
 * 3 words per voxel); 27 file bytes; 28 the validation's code (0 valid; the PackError of pack_host.hpp); 29 .. 31 zero.  Fields a failed validation did not reach are
 * zero.  Return 0 when the file opened and carries one of the two magics (valid or not: out32[1] says), -1 otherwise or for a null argument. */
int xs_host_checkpoint_info(const char *path, double *out32);

/* ---- Merging a second map into the volume (xs_tsdf_merge in xslam_amd.h: the per-voxel contract) ------------
 * T16: a real 4 x 4, row-major, taking a point of THIS map's volume frame (metres) to the OTHER map's volume frame, p_other = T p_this.
 * The other map is resampled into this map's voxel grid and averaged into it by weight, with this instance's max_integration_weight as the
 * cap; its resolution and voxel size may differ.  The device is drained first; afterwards the sign map, the cached planning and
 * relocalisation maps and the previous frame's model maps (at the current pose) follow the merged volume, as after xs_kf_load_checkpoint.
 * Poses, the frame number and the trajectory record are untouched.  *written (optional): the voxels written.
 * merge_volume: the source as device pointers at plane 0 of its three arrays, one pitch.  merge_map: the source is another instance of this
 * process (it is only read).  merge_checkpoint: the source is an XSTSDF2 file (xs_kf_save_checkpoint) of a whole volume, validated in
 * full before anything is touched (magic, exact length, shard_count 1, truncation distance), uploaded to a temporary device volume.
 * Return 1 when the merge ran, 0 without a volume, -1 on bad arguments with the state unchanged (a null or aliasing source, min_weight < 1,
 * an entry of T that is not finite, a bad file, a truncation distance different from this map's: stored values are normalised by it, so it
 * is refused, not rescaled), -2 in shard mode, doing nothing. */
int xs_kf_merge_volume(void *kf, const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res,
                       float src_voxel_size, float src_tranc_dist, const double *T16, int min_weight, unsigned long long *written);
int xs_kf_merge_map(void *kf, void *other_kf, const double *T16, int min_weight, unsigned long long *written);
int xs_kf_merge_checkpoint(void *kf, const char *path, const double *T16, int min_weight, unsigned long long *written);
/* ---- Taking fused frames out of the volume and fusing them again at corrected poses (xs_tsdf_reintegrate in
 * xslam_amd.h: the per-voxel contract) --------------------------------------------------------------------------------------------------------
 * n entries.  Entry i: the depth frame depth_dev[i] (u16 millimetres on the device, rows of step_bytes; entries may share a frame), mode[i] bit 0:
 * take it out of the volume at camera2volume c2v_old32xN + 32 i, bit 1: put it in at c2v_new32xN + 32 i (1: remove, 2: add, 3: move; both poses
 * [4, 4, 2] with their seeds; the array of a mode no entry asks for may be NULL).  frame_index (optional, n ints): an entry >= 0 replaces that
 * frame's stored world2camera by the pose that gives c2v_new (the entry must add), < 0 leaves the record alone.  The device is drained, every
 * distinct frame scaled once into a buffer of the call's own, the observations applied in entry order (an entry's removal before its addition)
 * in launches of at most XS_REINTEGRATE_MAX_OPS, with this instance's max_integration_weight and biInterpolate_threshold; afterwards the
 * volume's version is bumped and the sign map, the cached planning and relocalisation maps and the previous frame's model maps (at the current
 * pose) follow the edited volume, as after a merge: the next xs_kf_process_frame tracks against it.  The frame number and the number of poses
 * are untouched.  counts4 (optional) = {removed, added, emptied, orphaned} voxels over all observations.  A frame taken out of voxels whose
 * weight had reached max_integration_weight is removed only approximately (xslam_amd.h).
 * Return 1 when it ran, 0 without a volume, -1 on bad arguments with the state unchanged (n < 1, a null frame or array, a mode outside 1 .. 3, a
 * pose entry that is not finite, a frame index past the record or on an entry that does not add), -2 in shard mode, doing nothing. */
int xs_kf_reintegrate(void *kf, int n, const uint16_t *const *depth_dev, size_t step_bytes, const float *c2v_old32xN, const float *c2v_new32xN,
                      const int *mode, const int *frame_index, unsigned long long *counts4);
/* The host's side of a merge (x-slam_amd/host/merge_host.hpp).  CPU only.
 * merge_affine: xform12 of xs_tsdf_merge from T16 and the two voxel sizes, in float64 with one rounding to float32 at the end: the matrix
 * block is R vs_dst / vs_src, the offset (R (0.5 vs_dst (1, 1, 1)) + t) / vs_src - 0.5.  0, or -1 (nothing written) for an input that is
 * not finite or a voxel size that is not positive.
 * map_transform: T16 = c2v_other c2v_this^-1 for two real, rigid camera-to-volume poses (4 x 4, row-major) of the same camera frame: the
 * frame posed in this map, and in the other map by xs_kf_relocalize_global there, gives the T of a merge.  Returns 0.
 * merge_tile_box: the kernel's cull.  box6 = {lo x, y, z, hi x, y, z} (inclusive) contains every source voxel that a destination voxel of
 * the tile lo3 .. hi3 (inclusive) reads under xform12; returns 1, or 0 when no voxel of the tile falls inside the source. */
int xs_host_merge_affine(const double *T16, double dst_voxel_size, double src_voxel_size, float *out12);
int xs_host_map_transform(const double *c2v_this16, const double *c2v_other16, double *T16);
int xs_host_merge_tile_box(const float *xform12, const int *lo3, const int *hi3, const int *src_res, int *box6);

/* ---- Aligning a second map to the volume before merging it (xs_tsdf_align_terms in xslam_amd.h: the contract) --
 * Damped Gauss-Newton over the band index of THIS map on the residual "the other map, resampled at this map's band voxels under T, minus
 * this map": the samples, at the positions, that a merge under T would use.  T16xN: N >= 1 starting transforms, each a real 4 x 4, row-major,
 * as xs_kf_merge_map takes it; every start runs `iterations` damped steps ((J^T J + damping diag(J^T J)) delta = -J^T r, T <- exp(delta) T)
 * and one final pass that only reports the loss, the starts in one launch per pass.  A voxel takes part where the other map carries
 * min_weight on all eight corners around its sample and |residual| <= max_residual.  T16_out: the start that ended ok (at least six voxels on
 * every pass, the final loss pass included, and a positive definite system on every step) with the highest S = count - sum r^2,
 * relocalize_global's score (ties: the lower index).  S is a truncated-quadratic inlier score for max_residual <= 1 (every kept voxel adds
 * 1 - r^2 >= 0); with a larger max_residual a kept voxel can subtract more than it adds, and S then ranks by fit alone among starts that
 * all kept six voxels.  With iterations = 0 the one pass is the loss pass: a start that keeps fewer than six voxels does not end ok.
 * report8 = {the winner's index, its count, its sum r^2, its mean loss, launches run, starts that ended ok, band voxels in the index, 0}.
 * loss_history (optional, iterations + 1 doubles): the winner's mean loss per pass, the last entry the loss it ended at.
 * Nothing of either map is modified; the device is drained first.  align_map: the other map is another instance of this process.
 * align_checkpoint: an XSTSDF2 file of a whole volume, validated and uploaded as for xs_kf_merge_checkpoint.
 * Return 1; 0 without a volume or when no start ended ok (T16_out and loss_history untouched, report8[0] = -1); -1 on bad arguments (the
 * merge's, and N < 1, iterations < 0, damping negative or not finite, max_residual <= 0 or not finite, a source axis below 2); -2 in shard mode. */
int xs_kf_align_map(void *kf, void *other_kf, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                    double *T16_out, double *report8, double *loss_history);
int xs_kf_align_checkpoint(void *kf, const char *path, const double *T16xN, int N, int iterations, double damping, int min_weight, float max_residual,
                           double *T16_out, double *report8, double *loss_history);
/* The host's side of an alignment pass (x-slam_amd/host/align_host.hpp).  CPU only.
 * align_seeded_maps: out144 = six maps of 12 complex entries (re, im), xform12's order: T_k = (I + i h G_k) T through merge_affine's formula,
 * k = three translations then three rotations, h the seed step of the Gauss-Newton kernels.  The real parts are xs_host_merge_affine's bit
 * for bit for every k.  0, or -1 (nothing written): merge_affine's refusals.
 * align_step: s29 the scaled sums of a pass; solves (A + damping diag A) delta = -g by Cholesky and applies T16 <- exp(delta) T16 in float64.
 * 0 when the step was taken, -1 (T16 untouched) when count < 6 or the system is not positive definite. */
int xs_host_align_seeded_maps(const double *T16, double vs_this, double vs_other, float *out144);
int xs_host_align_step(const double *s29, double damping, double *T16);

/* ---- Scoring many map-to-map transforms, and alignment with no initial guess (xs_tsdf_score_transforms in
 * xslam_amd.h: the contract) ------------------------------------------------------------------------------------------------------------
 * score_transforms: {sum r^2, count} of "the other map resampled under T minus this map" over every stride-th entry of this map's band index
 * for each of the P transforms T16xP + 16 p (real 4 x 4, row-major, as xs_kf_merge_map takes T), in launches of 4096; out2xP + 2 p.  The
 * device is drained first; nothing of either map is modified.  Return 1; 0 without a volume; -1 on bad arguments (xs_kf_align_map's for the
 * other map, min_weight and max_residual, and P < 1, stride < 1, an entry of a T that is not finite); -2 in shard mode.
 *
 * align_map_global: xs_kf_align_map without a guess.  The two maps' band centroids give every candidate rotation its translation; round 0
 * scores opts->candidates transforms of xs_host_align_search_free (or the opts->user_n transforms of opts->user_T16xN, when given) and keeps
 * the opts->keep best by S = count - sum r^2; each of opts->rounds further rounds scores floor(candidates / keep) transforms of
 * xs_host_align_search_around about every kept one (pivot: this map's centroid; boxes refine_t and refine_r, halved per round; a kept
 * transform is entry 0 of its own group, so the best S never falls) and keeps the best again; the kept transforms then start
 * xs_kf_align_map's loop over the full band, whose winner and "ended ok" rule decide.
 * report12 = {the winner's rank after the last round, its S before refinement on the strided band, its count, sum r^2 and mean loss after
 * refinement, scoring launches run, alignment passes run, starts that ended ok, band voxels, scored entries per transform, the distance
 * of the other map's centroid from the image of this map's under the winner, 0}.
 * The score cannot tell a map from its image under a symmetry of the scene: a symmetric scene has several equally good answers.
 * opts NULL: the defaults, which xs_kf_align_search_defaults writes (box_t and refine_t: this map's truncation distance).  Otherwise every
 * field is taken as given.  Return codes: xs_kf_align_map's, including 0 with T16_out untouched when no start ends ok (or a map has no band
 * voxel); -1 also for a wrong struct_bytes, candidates < 1, keep outside 1 .. 32, rounds < 0, stride < 1, a box that is negative or not
 * finite, user_n < 0 or user_n > 0 without user_T16xN; -2 in shard mode.  Nothing of either map is modified. */
typedef struct xs_align_search_opts {
    unsigned struct_bytes;        /* sizeof(xs_align_search_opts) */
    int candidates;               /* 2048 */
    int keep;                     /* 8 (1 .. 32) */
    int rounds;                   /* 2 */
    int stride;                   /* 4 */
    int iterations;               /* 10 */
    int min_weight;               /* 1 */
    int user_n;                   /* 0 */
    double box_t;                 /* metres; the truncation distance */
    double refine_t;              /* metres; the truncation distance */
    double refine_r;              /* radians; 0.25 */
    double damping;               /* 1e-3 */
    double max_residual;          /* 1 */
    const double *user_T16xN;     /* NULL */
} xs_align_search_opts;
void xs_kf_align_search_defaults(void *kf, xs_align_search_opts *opts);
int xs_kf_score_transforms(void *kf, void *other_kf, int P, const double *T16xP, int stride, int min_weight, float max_residual, double *out2xP);
int xs_kf_score_transforms_checkpoint(void *kf, const char *path, int P, const double *T16xP, int stride, int min_weight, float max_residual,
                                      double *out2xP);
int xs_kf_align_map_global(void *kf, void *other_kf, const xs_align_search_opts *opts, double *T16_out, double *report12);
int xs_kf_align_checkpoint_global(void *kf, const char *path, const xs_align_search_opts *opts, double *T16_out, double *report12);
/* The host's side of the search (x-slam_amd/host/align_search_host.hpp).  CPU only, float64, deterministic.
 * align_search_free: candidate i = 0 .. n - 1 has the rotation of Shoemake's uniform-quaternion map at (halton(i + 1, 2), halton(i + 1, 3),
 * halton(i + 1, 5)) and the translation centroid_other - R centroid_this + box_t (2 halton(i + 1, {7, 11, 13}) - 1).
 * align_search_around: entry 0 is T16 itself; entry i >= 1, with u = 2 halton(i, {2, 3, 5, 7, 11, 13}) - 1, is T16 turned by
 * exp(box_r u[3:6]) (axis-angle) about the image of `pivot` under T16 and shifted by box_t u[0:3].
 * Both return 0, or -1 (nothing written) for n < 1, a null pointer, an input that is not finite or a negative box.
 * align_search_rank: the min(keep, P) indices with the highest S = count - sum r^2, best first, ties to the lower index; returns how many.
 * band_centroid: (sum / count + 0.5) voxel_size per axis from exact integer sums over packed keys (x | y << 21 | z << 42); 0, or -1 for no key. */
int xs_host_align_search_free(int n, const double *centroid_this3, const double *centroid_other3, double box_t, double *T16xN);
int xs_host_align_search_around(const double *T16, const double *pivot3, double box_t, double box_r, int n, double *T16xN);
int xs_host_align_search_rank(const double *out2xP, int P, int keep, int *idx_out);
int xs_host_band_centroid(const unsigned long long *keys, long long count, double voxel_size, double *out3);

/* ---- What differs between this map and a second map, as clusters (xs_tsdf_diff in xslam_amd.h: the contract) ----
 * T16 and the three sources as for the merge calls above (diff_volume needs no grad array); the same source validation, and another
 * truncation distance is refused.  THIS map is the instance's volume, the OTHER map the source resampled under T16.  A voxel is compared
 * where both maps carry min_weight (the other on every corner its sample needs); it is ONLY_THIS where this map's value is below lo and
 * the other's sample at least hi (matter here, firmly free there) and ONLY_OTHER the other way round (usual: lo = 0, hi = 0.5).  Each of the
 * two masks is labelled and clustered by the frontier's calls (26-adjacency within cells of `cell` voxels: 0, or a multiple of 8 in
 * 8 .. 65528) and the records of the clusters with count >= min_size come back in the frontier's format, ascending by label:
 * this_records8 / other_records8 (capacity x 8 uint64 each; may be null when capacity is 0), their numbers in *this_count / *other_count.
 * counts3 (optional): {compared, only_this, only_other} voxels.  this_dense / other_dense (optional, HOST, X * Y * Z bytes each): the masks
 * as one byte (0 or 1) per voxel, [(z Y + y) X + x].  With the other map the earlier one, only_this is what appeared and only_other what
 * went away.  The device is drained first.  Nothing of either map is modified: the volume generation, the sign map, the band index and the
 * planning caches stay, the call works in buffers of its own.
 * Return 1 when they ran, 0 without a volume, -1 on bad arguments with nothing written (the merge's, lo or hi not finite, lo > hi, a bad
 * cell, a negative capacity, null counts, a volume the frontier calls cannot label), -2 in shard mode, -4 with both needed counts in
 * *this_count / *other_count and nothing else written when capacity is too small for either list. */
int xs_kf_diff_volume(void *kf, const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size, float src_tranc_dist,
                      const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size, int capacity,
                      unsigned long long *this_records8, int *this_count, unsigned long long *other_records8, int *other_count, unsigned long long *counts3,
                      unsigned char *this_dense, unsigned char *other_dense);
int xs_kf_diff_map(void *kf, void *other_kf, const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size, int capacity,
                   unsigned long long *this_records8, int *this_count, unsigned long long *other_records8, int *other_count, unsigned long long *counts3,
                   unsigned char *this_dense, unsigned char *other_dense);
int xs_kf_diff_checkpoint(void *kf, const char *path, const double *T16, int min_weight, float lo, float hi, int cell, unsigned long long min_size, int capacity,
                          unsigned long long *this_records8, int *this_count, unsigned long long *other_records8, int *other_count,
                          unsigned long long *counts3, unsigned char *this_dense, unsigned char *other_dense);

/* Depth, normal and shaded views of a map from poses the caller picks (xs_render_views in xslam_amd.h: the contract).
 * `views` >= 1 camera2volume matrices c2v, 4 x 4 row-major: 16 floats each with complex_poses = 0, or 32 with complex_poses = 1 ((re, im) pairs as
 * xs_kf_get_camera2volume gives them; the real part is used).  Each renders a rows x cols image of a camera with intrinsics intr4 = {fx, fy, cx,
 * cy} (NULL: the configuration's; rows, cols = 0, 0: its image size) in launches of XS_RENDER_MAX_VIEWS views.  opts: an xs_render_opts of
 * xslam_amd.h, or NULL for the defaults (depths 0.2 .. 5.0 in steps of a voxel, min_weight 1, the cull on).  The outputs, each optional (NULL:
 * not wanted), view-major: depth float [views][rows][cols] in metres along the camera's z, 0 without a hit; depth_u16 the same in millimetres,
 * what xs_kf_process_frame and xs_kf_relocalize take; normal float [views][3][rows][cols] in the volume frame, NaN without one; shade uint8
 * [views][rows][cols]; counts4 unsigned [views][4] = {hit, backface, rejected, none}.  on_device = 0: host arrays; 1: device arrays, written
 * in place.  The device is drained before and the stream after: the outputs are complete on return.  Nothing of any map is modified.
 * render_views renders this instance's map; the brick mask of the cull is cached and follows the volume like the observation grid.
 * render_volume, render_map and render_checkpoint render a second map (the caller's arrays; another instance; a checkpoint of a whole volume in
 * either format), as the merge obtains it, with its own resolution and voxel size.
 * Return 1, 0 without a volume, -1 on bad arguments (views < 1, a null c2v, every output null, what xs_render_views refuses, a second map the
 * merge would refuse) with nothing written, -2 in shard mode. */
struct xs_render_opts;
int xs_kf_render_views(void *kf, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols, const struct xs_render_opts *opts,
                       float *depth, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device);
int xs_kf_render_volume(void *kf, const float *src_value, const int *src_weight, size_t src_step, const int *src_res, float src_voxel_size, float src_tranc_dist,
                        int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols, const struct xs_render_opts *opts, float *depth,
                        uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device);
int xs_kf_render_map(void *kf, void *other_kf, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols,
                     const struct xs_render_opts *opts, float *depth, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4, int on_device);
int xs_kf_render_checkpoint(void *kf, const char *path, int views, const float *c2v, int complex_poses, const float *intr4, int rows, int cols,
                            const struct xs_render_opts *opts, float *depth, uint16_t *depth_u16, float *normal, unsigned char *shade, unsigned *counts4,
                            int on_device);

/* The map asked at points the caller supplies, and at the pixels of a depth frame (xs_tsdf_sample_points and
 * xs_tsdf_sample_depth in xslam_amd.h: the contract).  points: n x 3 floats in metres, 1 <= n <= 2^30, in a frame that T16 (a real 4 x 4,
 * row-major; NULL: none, the points' bits are used as they are) takes to the sampled map's volume frame.  A voxel with a weight below
 * min_weight (below 1: 1) is unseen.  The outputs, each optional (NULL: not wanted): status uint8 [n] (0 outside, 1 unseen, 2 ok, 3 no
 * depth); value float [n], the trilinear value in units of the truncation distance, NaN where the status is not ok; dvalue float [n], the
 * grad array interpolated the same way; gradient float [n][3] in value per metre; counts4 unsigned long long [4] = {outside, unseen, ok,
 * no_depth}.  on_device bit 0: the points (the depth image) are device memory; bit 1: the outputs are, and are written in place.  The device
 * is drained before and the stream after: the outputs are complete on return.  Nothing of any map or cache is modified.
 * sample_points asks this instance's map; sample_volume, sample_map and sample_checkpoint a second map (the caller's arrays, src_grad only
 * where dvalue is wanted; another instance; a checkpoint of a whole volume in either format), as the render calls obtain it.
 * frame_residuals asks this map at the points of a depth image (u16 millimetres, depth_step bytes per row, 0: packed) seen from the
 * camera2volume c2v (16 floats, or 32 with complex_poses = 1: the real parts) with intrinsics intr4 (NULL: the configuration's; rows, cols =
 * 0, 0: its image size): the outputs are images [rows][cols], the gradient [3][rows][cols], and value is the frame's signed residual
 * against the map at that pose.
 * Return 1, 0 without a volume, -1 on bad arguments (what the kernels' calls refuse, a T16 entry that is not finite, a second map the
 * merge would refuse) with nothing written, -2 in shard mode (a point's eight corners may straddle two ranks' slabs).
 * xs_host_sample_compose: T16 = T_a2v16 T_p2a16 for points given in a frame P whose pose in frame A is T_p2a, A's in the volume T_a2v
 * (affine, float64; host only); 0, -1 for a null pointer. */
int xs_kf_sample_points(void *kf, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value, float *dvalue,
                        float *gradient, unsigned long long *counts4, int on_device);
int xs_kf_sample_volume(void *kf, const float *src_value, const int *src_weight, const float *src_grad, size_t src_step, const int *src_res, float src_voxel_size,
                        float src_tranc_dist, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                        float *dvalue, float *gradient, unsigned long long *counts4, int on_device);
int xs_kf_sample_map(void *kf, void *other_kf, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                     float *dvalue, float *gradient, unsigned long long *counts4, int on_device);
int xs_kf_sample_checkpoint(void *kf, const char *path, long long n, const float *points, const double *T16, int min_weight, unsigned char *status, float *value,
                            float *dvalue, float *gradient, unsigned long long *counts4, int on_device);
int xs_kf_frame_residuals(void *kf, const unsigned short *depth, size_t depth_step, const float *c2v, int complex_poses, const float *intr4, int rows, int cols,
                          int min_weight, unsigned char *status, float *value, float *dvalue, float *gradient, unsigned long long *counts4, int on_device);
int xs_host_sample_compose(const double *T_a2v16, const double *T_p2a16, double *T16);

/* A point cloud registered to a map (xs_tsdf_register_terms in xslam_amd.h: the contract).  Damped Gauss-Newton on
 * the residual "the map's value at T p" over the n points (n x 3 floats in metres, 1 <= n <= 2^30; on_device bit 0: device memory): the
 * transform T (cloud frame to the map's volume frame) that puts the cloud on the map's surface.  T16xN: N >= 1 starting transforms, each a
 * real 4 x 4, row-major; every start runs `iterations` damped steps ((J^T J + damping diag(J^T J)) delta = -J^T r, T <- exp(delta) T in
 * float64, each pass's transforms rounded once to float32 for the kernel) and one final pass that only reports the loss, the starts in one
 * launch per pass.  A point takes part where the map's value and its gradient exist at T p with min_weight and |value| <= max_residual.
 * T16_out: the start that ended ok (at least six points on every pass, the final loss pass included, and a positive definite system on every
 * step) with the highest S = count - sum r^2 (ties: the lower index): xs_kf_align_map's rule, iterations = 0 included.
 * report7 = {the winner's index, its count, its sum r^2, its mean loss, launches run, starts that ended ok, n}.  loss_history (optional,
 * iterations + 1 doubles): the winner's mean loss per pass.
 * register_points asks this instance's map; register_map another instance's; register_checkpoint a checkpoint of a whole volume in either
 * format.  The device is drained before and the stream after.  Nothing of any map or cache is modified; xs_kf_volume_generation stays.
 * Return codes: xs_kf_align_map's: 1; 0 without a volume or when no start ended ok (T16_out and loss_history untouched, report7[0] = -1);
 * -1 on bad arguments (n outside 1 .. 2^30, a null pointer, N < 1, iterations < 0, min_weight < 1, damping negative or not finite,
 * max_residual <= 0 or not finite, a start that is not finite in float32, a second map the merge would refuse); -2 in shard mode.
 * xs_host_register_step: xs_host_align_step on the kernel's sums as they stand (no scaling); 0, or -1 with T16 untouched.  CPU only. */
int xs_kf_register_points(void *kf, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations, double damping,
                          int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history);
int xs_kf_register_map(void *kf, void *other_kf, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations,
                       double damping, int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history);
int xs_kf_register_checkpoint(void *kf, const char *path, long long n, const float *points, int on_device, const double *T16xN, int N, int iterations,
                              double damping, int min_weight, float max_residual, double *T16_out, double *report7, double *loss_history);
int xs_host_register_step(const double *s29, double damping, double *T16);

/* ---- Scoring many transforms of a point cloud, and registration with no starting guess (xs_tsdf_score_points in
 * xslam_amd.h: the contract) ------------------------------------------------------------------------------------------------------------
 * score_point_transforms: {sum r^2, count} of "the map's value at T p" over every stride-th of the n points (as xs_kf_register_points takes
 * them) for each of the P transforms T16xP + 16 p (real 4 x 4, row-major: cloud frame to the map's volume frame, each rounded once to
 * float32 as xs_kf_register_points rounds its starts), in launches of 4096; out2xP + 2 p.  No gradient gate: a point counts wherever the map
 * holds a value at T p with min_weight and |value| <= max_residual.  score_point_transforms asks this instance's map, _map another
 * instance's, _checkpoint a checkpoint of a whole volume in either format.  The device is drained before and the stream after; nothing of
 * any map or cache is modified.  Return 1; 0 without a volume; -1 on bad arguments (n outside 1 .. 2^30, a null pointer, P < 1, stride < 1,
 * min_weight < 1, max_residual <= 0 or not finite, a T that is not finite in float32, a second map the merge would refuse); -2 in shard mode.
 *
 * register_points_global: xs_kf_register_points without a guess.  The cloud's centroid (xs_host_points_centroid over the scored points) and
 * the map's band centroid give every candidate rotation its translation; round 0 scores opts->candidates transforms of
 * xs_host_align_search_free with "this" = the cloud and "other" = the map (or the opts->user_n transforms of opts->user_T16xN, when given)
 * and keeps the opts->keep best by S = count - sum r^2; each of opts->rounds further rounds scores floor(candidates / keep) transforms of
 * xs_host_align_search_around about every kept one (pivot: the cloud's centroid; boxes refine_t and refine_r, halved per round; a kept
 * transform is entry 0 of its own group, so the best S never falls) and keeps the best again: xs_kf_align_map_global's rounds and ranking.
 * The kept transforms then start xs_kf_register_points' loop over ALL n points, whose winner and "ended ok" rule decide.
 * report12 = {the winner's rank after the last round, its S before refinement on the strided cloud, its count, sum r^2 and mean loss after
 * refinement, scoring launches run, registration passes run, starts that ended ok, n, scored points per transform, the distance of the
 * map's band centroid from the image of the cloud's centroid under the winner, 0}.
 * The score cannot tell a scene from its image under one of its own symmetries: a symmetric scene has several equally good answers.
 * opts NULL: the defaults, which xs_kf_register_search_defaults writes (box_t and refine_t: the map's truncation distance; max_residual 0.9,
 * xs_kf_register_points' usual one: a point in seen free space has r = 1 and adds nothing to S at 0.9 or at 1).  Otherwise every field is
 * taken as given.  Return codes: xs_kf_register_points', including 0 with T16_out untouched when no start ends ok or the map has no band
 * voxel; -1 also for a wrong struct_bytes, candidates < 1, keep outside 1 .. 32, rounds < 0, stride < 1, a box that is negative or not
 * finite, user_n < 0 or user_n > 0 without user_T16xN, and for ceil(n / stride) > 2^24 scored points (raise the stride: the search needs no
 * more, and the final loop runs over all n regardless); -2 in shard mode.  Nothing of any map or cache is modified;
 * xs_kf_volume_generation stays.
 * xs_host_points_centroid: the mean of points stride i, i = 0 .. ceil(n / stride) - 1 (host array, n x 3 floats), each axis added in
 * double in index order and divided by the scored count; 0, or -1 (nothing written) for n < 1, stride < 1 or a null pointer.  CPU only. */
typedef struct xs_register_search_opts {
    unsigned struct_bytes;        /* sizeof(xs_register_search_opts) */
    int candidates;               /* 2048 */
    int keep;                     /* 8 (1 .. 32) */
    int rounds;                   /* 2 */
    int stride;                   /* 4 */
    int iterations;               /* 10 */
    int min_weight;               /* 1 */
    int user_n;                   /* 0 */
    double box_t;                 /* metres; the truncation distance */
    double refine_t;              /* metres; the truncation distance */
    double refine_r;              /* radians; 0.25 */
    double damping;               /* 1e-3 */
    double max_residual;          /* 0.9 */
    const double *user_T16xN;     /* NULL */
} xs_register_search_opts;
void xs_kf_register_search_defaults(void *kf, xs_register_search_opts *opts);
int xs_kf_score_point_transforms(void *kf, long long n, const float *points, int on_device, int P, const double *T16xP, int stride, int min_weight,
                                 float max_residual, double *out2xP);
int xs_kf_score_point_transforms_map(void *kf, void *other_kf, long long n, const float *points, int on_device, int P, const double *T16xP, int stride,
                                     int min_weight, float max_residual, double *out2xP);
int xs_kf_score_point_transforms_checkpoint(void *kf, const char *path, long long n, const float *points, int on_device, int P, const double *T16xP,
                                            int stride, int min_weight, float max_residual, double *out2xP);
int xs_kf_register_points_global(void *kf, long long n, const float *points, int on_device, const xs_register_search_opts *opts, double *T16_out,
                                 double *report12);
int xs_kf_register_points_global_map(void *kf, void *other_kf, long long n, const float *points, int on_device, const xs_register_search_opts *opts,
                                     double *T16_out, double *report12);
int xs_kf_register_points_global_checkpoint(void *kf, const char *path, long long n, const float *points, int on_device,
                                            const xs_register_search_opts *opts, double *T16_out, double *report12);
int xs_host_points_centroid(const float *points, long long n, int stride, double *out3);

/* A registered point cloud fused into this instance's map (xs_tsdf_fuse_points_accumulate and xs_tsdf_fuse_points_fold
 * in xslam_amd.h: the contract).  points: n x 3 floats in metres (n >= 1; on_device bit 0: device memory) and origin3, the sensor's position,
 * in a frame that T16 (real 4 x 4, row-major, as xs_kf_register_points returns it; NULL: the volume frame, the bits as they are) takes to the
 * volume frame.  Each point's ray is walked in half-voxel steps from at most the truncation distance in front of the point (carve != 0: from
 * the sensor) to the truncation distance behind it; every voxel entered receives the signed distance to the point along the ray, in units of
 * the truncation distance and clamped at 1.  A voxel receives ONE observation of weight `weight` (1 .. the configuration's
 * max_integration_weight) per run of at most 2^24 - 1 points, the mean over the rays that entered it, averaged in as a depth frame's is.  Rays
 * shorter than min_range (> 0) or longer than max_range are dropped.  The result does not depend on the order of the points.
 * counts5 (optional) = {points used, points dropped, visits, samples outside the volume, voxels written}.  Afterwards everything derived
 * from the volume follows as after xs_kf_reintegrate; xs_kf_volume_generation advances; poses and the frame number stay.  The accumulator
 * (8 bytes per voxel) is allocated on first use and kept; xs_kf_release_fuse_scratch frees it.
 * Return 1, 0 without a volume, -1 on bad arguments (a null pointer, n < 1, an entry that is not finite, min_range <= 0, max_range <
 * min_range or above 2^19 voxels, a weight outside its range, a truncation distance above 128 voxels) with the state unchanged, -2 in shard
 * mode. */
int xs_kf_fuse_points(void *kf, long long n, const float *points, int on_device, const double *T16, const float *origin3, float min_range, float max_range,
                      int carve, int weight, unsigned long long *counts5);
void xs_kf_release_fuse_scratch(void *kf);

/* ---- The reference's own call shape (x-slam_amd/host/reference_shape.hpp) ---------------------------------------------------------
 * The per-frame sequence of Experiments/test_xkinect_fusion/main.cpp:46-60 + KinectFusionReconstruction.cpp:147-332 over nothing but the
 * reference-signature launchers (bilateralFilter, pyrDown, createVMap / createNMap, estimateCombined per iteration, integrateTsdfVolume,
 * raycast, resizeVMap / resizeNMap — x-slam_amd/host/xs_launchers.hpp) with the reference's argument lists and a stream drain wherever
 * the reference's launcher drains the device: what swapping the library and changing nothing else gives.  Same results as xs_kf_* bit
 * for bit (tests/test_reference_shape_gpu.py); bench.py times it as legs.reference_call_shape.  Config: the same flat YAML. */
void *xs_refshape_create(const char *yaml_text);
void xs_refshape_destroy(void *rs);
/* main.cpp:50-58: DeviceArray2D<ushort>::upload of a host frame (dense rows), then ProcessFrame */
int xs_refshape_process_frame_host(void *rs, const uint16_t *depth_host);
/* ProcessFrame on a frame already in device memory (main.cpp:57-60 times ProcessFrame alone) */
int xs_refshape_process_frame(void *rs, const uint16_t *depth_dev, size_t step_bytes);
int xs_refshape_frame_id(void *rs);
void xs_refshape_get_world2camera(void *rs, int idx, float *out32);
int xs_refshape_download_volume(void *rs, float *value, int *weight, float *grad);
int xs_refshape_download_map(void *rs, int which, int level, float *out);   /* as xs_kf_download_map */
/* per ICP iteration of the last frame: the 54 sums estimateCombined returned (no inlier count: ICP.h:24-31 has none); returns #doubles */
int xs_refshape_icp_log(void *rs, double *out, int capacity);
/* ComputeLocalTsdf_hessian / ComputeLocalTsdf_loss through their TsdfFusion.h:48-60 signatures (PtrStepSz<ushort> depth on the device,
 * MatD33 = 36 floats / devDComplex3 = 12 floats, or Mat33 = 9 / float3 = 3; gt_dev: X*Y*Z floats, dense).  out4 = the returned float4
 * {loss, gradient, second derivative, count}, out2 = float2 {loss, count}.  with_volumes: the per-voxel scratch volumes of the reference's
 * thrust vectors are filled too and copied to volumes_host (real | grad | hessian | count as int32: 4 x N^3 words; loss: real | count). */
int xs_refshape_hessian(const uint16_t *depth_dev, size_t depth_step, int rows, int cols, const float *intr4, const int *res3, float voxel_size,
                        const float *Rv2c36, const float *tv2c12, float tranc_dist, const float *gt_dev, int with_volumes, float *out4,
                        float *volumes_host);
int xs_refshape_loss(const uint16_t *depth_dev, size_t depth_step, int rows, int cols, const float *intr4, const int *res3, float voxel_size,
                     const float *Rv2c9, const float *tv2c3, float tranc_dist, const float *gt_dev, int with_volumes, float *out2,
                     float *volumes_host);

#ifdef __cplusplus
}
#endif
#endif
